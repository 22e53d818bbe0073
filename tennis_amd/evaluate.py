"""Evaluation / feature-extraction driver — mirror of reference evaluate.py for the
hot path: same flag names, ``save_features`` (evaluate.py:306-321) and
``evaluate_model`` (evaluate.py:274-303) with the same results.

Differences that are deliberate: one device per rank
(no serialised per-device inner loop, no ``idxs`` rebinding bug), one D2H copy per
batch instead of one per row, frames sharded by batch across ranks.

``--num_gpus N`` (reference evaluate.py:101-102: the ``ctx`` list each batch is split over) starts N processes of
this script, one per GPU (``sharding.launch``; under ``torch.distributed.run`` the ranks exist already):
``--save_feats`` then goes through ``save_features_sharded`` — every rank encodes its batches, writes their
``.npy`` files and the feature rows are all-gathered over RCCL so that each rank ends with the whole (N, F)
matrix; testing shards the batches and sums the confusion matrices.  ``--corpus_frames N`` runs BASELINE config
C4 — a synthetic N-frame corpus (786 455 = the 5-match corpus) through the same sharded encode +
chunked, overlapped all-gather — and prints one JSON line with the rates.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import sharding, transforms
from .events import check_save_events, decode_split, event_table, save_events
from .dataset import DataLoader, TennisSet
from .metrics.vision import PRF1
from .model_zoo import get_model
from .models.vision.definitions import CNNRNN, FrameModel, TemporalPooling


def _keep_logits(keep, outputs, idxs):
    """``keep`` (a dict, or None: nothing happens) collects what ``--save_events`` decodes: the device logits of every batch and the
    dataset index of every row, in loader order."""
    if keep is not None:
        keep.setdefault("logits", []).append(outputs)
        keep.setdefault("order", []).extend(int(j) for j in idxs)


def evaluate_model(net, loader, dataset, metrics, ctx=None, keep=None):
    """Reference evaluate.py:274-303: forward, metric.update, results[img_path] = raw
    logits, ground_truths[img_path] = class index.  ``keep``: ``_keep_logits``."""
    results, ground_truths = dict(), dict()
    for data, labels, idxs in loader:
        outputs = net(data)
        _keep_logits(keep, outputs, idxs)
        lab = torch.from_numpy(labels).to(outputs.device)
        for metric in metrics:
            metric.update([lab], [outputs])
        out = outputs.cpu().numpy()
        for i, idx in enumerate(int(j) for j in idxs):
            sample = dataset._samples[idx]
            img_path = dataset.get_image_path(dataset._frames_dir, sample[0], sample[1])
            results[img_path] = out[i]
            ground_truths[img_path] = dataset.classes.index(sample[2])
    return results, ground_truths


def check_save_cams(flags, world=1):
    """``--save_cams`` is for a frame model on one rank: exits with the reason otherwise.  Touches no device."""
    if not getattr(flags, "save_cams", False):
        return
    if flags.window != 1:
        raise SystemExit("--save_cams needs a frame model: --window %d evaluates a temporal model, and past a recurrent layer or a pool "
                         "over windows a logit is no longer a sum over the cells of one frame's map" % flags.window)
    if flags.feats_model is not None:
        raise SystemExit("--save_cams needs the frames: --feats_model evaluates stored features, the last feature map is not there")
    if flags.temp_pool is not None:
        raise SystemExit("--save_cams needs a frame model: --temp_pool %s pools over frames" % flags.temp_pool)
    if flags.save_feats:
        raise SystemExit("--save_cams writes the maps of a test run: not together with --save_feats")
    if flags.dense_windows or flags.corpus_frames > 0:
        raise SystemExit("--save_cams needs a frame model: not together with --dense_windows / --corpus_frames")
    if flags.num_gpus > 1 or world > 1:
        raise SystemExit("--save_cams writes one file from one rank: run it with --num_gpus 1")


def evaluate_model_cams(net, loader, dataset, metrics, keep=None):
    """``evaluate_model`` of a ``FrameModel`` through ``forward(x, return_cam=True)``: the same logits (bit for bit), the same
    metric updates and return values, and as a third value the columns of ``save_cams`` in loader order - per frame the map of
    its arg-max class ``cam (N, h, w)``, ``pred``, ``label``, that class's ``logit``, ``video`` and ``frame``."""
    results, ground_truths = dict(), dict()
    cols = {k: [] for k in ("cam", "pred", "label", "logit", "video", "frame")}
    for data, labels, idxs in loader:
        outputs, cam = net(data, return_cam=True)
        _keep_logits(keep, outputs, idxs)
        lab = torch.from_numpy(labels).to(outputs.device)
        for metric in metrics:
            metric.update([lab], [outputs])
        pred = outputs.argmax(1)
        rows = torch.arange(outputs.shape[0], device=outputs.device)
        cols["cam"].append(cam[rows, pred].cpu().numpy())
        cols["pred"].append(pred.cpu().numpy())
        out = outputs.cpu().numpy()
        cols["logit"].append(out[np.arange(len(out)), cols["pred"][-1]])
        for i, idx in enumerate(int(j) for j in idxs):
            sample = dataset._samples[idx]
            img_path = dataset.get_image_path(dataset._frames_dir, sample[0], sample[1])
            results[img_path] = out[i]
            ground_truths[img_path] = dataset.classes.index(sample[2])
            cols["label"].append(ground_truths[img_path])
            cols["video"].append(sample[0])
            cols["frame"].append(int(sample[1]))
    for k in ("cam", "pred", "logit"):
        cols[k] = np.concatenate(cols[k])
    return results, ground_truths, cols


def save_cams(file_path, cam, pred, label, logit, video, frame):
    """One ``.npz`` of flat arrays (``np.load(..., allow_pickle=False)`` reads it): ``cam (N, h, w)`` float32 the class activation
    map of each frame's arg-max class, ``pred (N,)`` that class, ``label (N,)``, ``logit (N,)`` its logit
    (= the Dense bias of ``pred`` + ``cam.sum((1, 2))``), ``video (N,)`` unicode and ``frame (N,)`` the frame number."""
    cam = np.ascontiguousarray(cam, np.float32)
    n = len(cam)
    if cam.ndim != 3:
        raise ValueError(f"save_cams: cam must be (N, h, w), got {cam.shape}")
    cols = dict(cam=cam, pred=np.asarray(pred, np.int64).reshape(-1), label=np.asarray(label, np.int64).reshape(-1),
                logit=np.asarray(logit, np.float32).reshape(-1), video=np.asarray(list(video), dtype=np.str_).reshape(-1),
                frame=np.asarray(frame, np.int64).reshape(-1))
    for k, v in cols.items():
        if len(v) != n:
            raise ValueError(f"save_cams: {k} has {len(v)} entries for {n} maps")
    os.makedirs(os.path.dirname(os.path.abspath(file_path)), exist_ok=True)
    np.savez(file_path, **cols)


def load_cams(file_path):
    """-> dict of ``save_cams``' arrays: ``cam``, ``pred``, ``label``, ``logit``, ``video``, ``frame``."""
    with np.load(file_path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    missing = [k for k in ("cam", "pred", "label", "logit", "video", "frame") if k not in d]
    if missing:
        raise ValueError(f"{file_path}: not a file of save_cams (no {', '.join(missing)})")
    return d


def check_save_tams(flags, world=1):
    """``--save_tams`` is for a windowed model that ends in ``max over the window -> Dense``, on one rank: exits with the reason
    otherwise.  Touches no device."""
    if not getattr(flags, "save_tams", False):
        return
    if flags.window <= 1:
        raise SystemExit("--save_tams needs a temporal model: --window %d evaluates single frames, there is no window whose steps a "
                         "logit could be read from (--save_cams maps a frame model's logits onto the frame)" % flags.window)
    if flags.temp_pool == "mean":
        raise SystemExit("--save_tams needs --temp_pool gru|lstm|max: a mean reads every step alike - its maps are the Dense applied to "
                         "each step's features divided by the window, which needs no run of this driver")
    if flags.temp_pool not in ("gru", "lstm", "max"):
        raise SystemExit("--save_tams needs --temp_pool gru|lstm|max, got %r" % flags.temp_pool)
    if flags.save_feats:
        raise SystemExit("--save_tams writes the maps of a test run: not together with --save_feats")
    if flags.corpus_frames > 0:
        raise SystemExit("--save_tams writes the maps of a split's samples: --corpus_frames runs a synthetic corpus that has none")
    if flags.num_gpus > 1 or world > 1:
        raise SystemExit("--save_tams writes one file from one rank: run it with --num_gpus 1")


TAM_COLUMNS = ("tam", "pred", "label", "logit", "video", "frame", "frames", "bias")


def tam_columns(net, dataset, order, outputs, tam):
    """The columns of ``save_tams`` for the samples ``order`` (dataset indices) with logits ``outputs`` (N, classes) and maps ``tam``
    (N, classes, window) in that order: per sample the map of its arg-max class ``tam (N, window)``, ``pred``, ``label``, that class's
    ``logit`` and Dense ``bias``, ``video``, the centre ``frame`` and ``frames (N, window)``, the frame number every window step read
    (``TennisSet.window_frames``)."""
    pred = outputs.argmax(1)
    rows = torch.arange(outputs.shape[0], device=outputs.device)
    sel, pred, out = tam[rows, pred].cpu().numpy(), pred.cpu().numpy(), outputs.cpu().numpy()
    bias = np.asarray(net.classes._own_params[net.classes.prefix + "bias"].data, np.float32).reshape(-1)
    samples = [dataset._samples[int(i)] for i in order]
    return dict(tam=sel, pred=pred, label=[dataset.classes.index(s[2]) for s in samples], logit=out[np.arange(len(out)), pred],
                video=[s[0] for s in samples], frame=[int(s[1]) for s in samples],
                frames=np.asarray([dataset.window_frames(s) for s in samples], np.int64).reshape(len(samples), -1), bias=bias[pred])


def evaluate_model_tams(net, loader, dataset, metrics, keep=None):
    """``evaluate_model`` of a windowed ``CNNRNN`` / ``TemporalPooling(max)`` through ``forward(x, return_tam=True)``: the same
    logits (bit for bit), metric updates and return values, and as a third value the columns of ``save_tams`` in loader order."""
    results, ground_truths = dict(), dict()
    outs, tams, order = [], [], []
    for data, labels, idxs in loader:
        outputs, tam = net(data, return_tam=True)
        _keep_logits(keep, outputs, idxs)
        lab = torch.from_numpy(labels).to(outputs.device)
        for metric in metrics:
            metric.update([lab], [outputs])
        outs.append(outputs)
        tams.append(tam)
        out = outputs.cpu().numpy()
        for i, idx in enumerate(int(j) for j in idxs):
            sample = dataset._samples[idx]
            img_path = dataset.get_image_path(dataset._frames_dir, sample[0], sample[1])
            results[img_path] = out[i]
            ground_truths[img_path] = dataset.classes.index(sample[2])
            order.append(idx)
    return results, ground_truths, tam_columns(net, dataset, order, torch.cat(outs), torch.cat(tams))


def save_tams(file_path, tam, pred, label, logit, video, frame, frames, bias):
    """One ``.npz`` of flat arrays (``np.load(..., allow_pickle=False)`` reads it): ``tam (N, window)`` float32 the temporal activation
    map of each sample's arg-max class, ``pred (N,)`` that class, ``label (N,)``, ``logit (N,)`` its logit (= ``bias`` +
    ``tam.sum(1)``), ``bias (N,)`` the Dense bias of ``pred``, ``video (N,)`` unicode, ``frame (N,)`` the centre frame and
    ``frames (N, window)`` the frame number every window step read.  ``tam[n, t]`` is what the logit read from the model's state at
    window step ``t``; a recurrent state at step ``t`` has seen the steps before it (after it, in the reverse direction), so this
    names the step whose state was read, not a single frame that caused the logit."""
    tam = np.ascontiguousarray(tam, np.float32)
    n = len(tam)
    if tam.ndim != 2:
        raise ValueError(f"save_tams: tam must be (N, window), got {tam.shape}")
    cols = dict(tam=tam, pred=np.asarray(pred, np.int64).reshape(-1), label=np.asarray(label, np.int64).reshape(-1),
                logit=np.asarray(logit, np.float32).reshape(-1), video=np.asarray(list(video), dtype=np.str_).reshape(-1),
                frame=np.asarray(frame, np.int64).reshape(-1), frames=np.asarray(frames, np.int64).reshape(n, -1),
                bias=np.asarray(bias, np.float32).reshape(-1))
    for k, v in cols.items():
        if len(v) != n:
            raise ValueError(f"save_tams: {k} has {len(v)} entries for {n} maps")
    if cols["frames"].shape != tam.shape:
        raise ValueError(f"save_tams: frames must be {tam.shape} like tam, got {cols['frames'].shape}")
    os.makedirs(os.path.dirname(os.path.abspath(file_path)), exist_ok=True)
    np.savez(file_path, **cols)


def load_tams(file_path):
    """-> dict of ``save_tams``' arrays: ``tam``, ``pred``, ``label``, ``logit``, ``video``, ``frame``, ``frames``, ``bias``."""
    with np.load(file_path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    missing = [k for k in TAM_COLUMNS if k not in d]
    if missing:
        raise ValueError(f"{file_path}: not a file of save_tams (no {', '.join(missing)})")
    return d


def load_feature_matrix(dataset):
    """The dataset-order (len(dataset), F) feature matrix from the ``.npy`` files of ``dataset.feat_dir``: every frame's file is
    read once (the loader path reads it once per window that contains it)."""
    rows = [np.load(dataset.get_feature_path(dataset.feat_dir, s[0], s[1])).astype(np.float32).reshape(-1) for s in dataset._samples]
    return np.stack(rows)


TABLE_LOAD_THREADS = 8      # host threads of load_feature_table: file reads overlap; a constant, not the machine's core count


def read_rows(read, n):
    """(n, F) float32: row r = ``read(r)`` flattened, every r read once on the table readers' thread pool (row 0 first, for the width)."""
    first = np.asarray(read(0), np.float32).reshape(-1)
    table = np.empty((n, first.size), np.float32)
    table[0] = first

    def fill(r):
        table[r] = np.asarray(read(r)).reshape(-1)

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=TABLE_LOAD_THREADS) as pool:
        list(pool.map(fill, range(1, n)))
    return table


def load_feature_table(dataset, frames):
    """The (len(frames), F) float32 feature table of ``TennisSet.window_table``: row r is the ``.npy`` of ``frames[r]`` = (video,
    frame) under ``dataset.feat_dir``, every file read exactly once (the loader path reads it about ``window`` times per epoch)."""
    if not len(frames):
        raise ValueError("load_feature_table: no frames")
    path = lambda vf: dataset.get_feature_path(dataset.feat_dir, vf[0], vf[1])
    return read_rows(lambda r: np.load(path(frames[r])), len(frames))


def evaluate_windows(net, dataset, metrics, features=None, batch_size=65536, return_tams=False, keep=None):
    """``evaluate_model`` for a windowed feature-mode model (``CNNRNN`` / ``TemporalPooling``) without the loader: the
    dataset-order feature matrix (``features``: (len(dataset), F), e.g. what ``save_features_sharded`` returned; None: loaded from
    the ``.npy`` files, each once) goes to the device once, ``net.forward_windows`` evaluates every sample's window from it
    (``TennisSet.window_rows``), and the metrics are updated in dataset order in pieces of ``batch_size``.  Same return values:
    results[img_path] = raw logits, ground_truths[img_path] = class index; ``return_tams``: the columns of ``save_tams`` as a third,
    from ``forward_windows(..., return_tam=True)`` (the same logits)."""
    centre, lo, hi, row_stride = dataset.window_rows()
    if features is None:
        features = load_feature_matrix(dataset)
    if len(features) != len(dataset):
        raise ValueError(f"evaluate_windows: {len(features)} feature rows for {len(dataset)} samples")
    outputs = net.forward_windows(features, centre, lo, hi, dataset._window, row_stride, return_tam=return_tams)
    if return_tams:
        outputs, tam = outputs
    _keep_logits(keep, outputs, range(len(dataset)))
    labels = torch.tensor([dataset.classes.index(s[2]) for s in dataset._samples], dtype=torch.float32, device=outputs.device)
    for a in range(0, len(dataset), batch_size):
        for metric in metrics:
            metric.update([labels[a:a + batch_size]], [outputs[a:a + batch_size]])
    out = outputs.cpu().numpy()
    results, ground_truths = dict(), dict()
    for i, sample in enumerate(dataset._samples):
        img_path = dataset.get_image_path(dataset._frames_dir, sample[0], sample[1])
        results[img_path] = out[i]
        ground_truths[img_path] = dataset.classes.index(sample[2])
    if return_tams:
        return results, ground_truths, tam_columns(net, dataset, range(len(dataset)), outputs, tam)
    return results, ground_truths


def encode_table(net_backbone, dataset, frames, batch_size=64, num_workers=0):
    """The (len(frames), F) float32 DEVICE feature table of ``TennisSet.window_table`` for a model on frames: row r is
    ``net_backbone`` applied to frame ``frames[r]`` = (video, frame).  Every frame is loaded (the dataset's own decode / transform
    route, ``TennisSet.frame_view`` under the same ``DataLoader``) and encoded exactly once, in batches of ``batch_size``; the
    encoder writes a batch's rows straight into the table (its ``out=``) and nothing waits for them, so the loader reads and
    decodes the next batch behind the encode of this one (as ``save_features_sharded``'s file writes run behind it).  No ``.npy``
    is read or written."""
    from .nn import _to_device
    if not len(frames):
        raise ValueError("encode_table: no frames")
    loader = DataLoader(dataset.frame_view(frames), batch_size=batch_size, shuffle=False, num_workers=num_workers)
    table, r0, shape = None, 0, None
    for data, _labels, _idxs in loader:
        x = _to_device(data)
        n = x.shape[0]
        eng = getattr(net_backbone, "_engine", None)
        if table is not None and tuple(x.shape[1:]) == shape and hasattr(eng, "feature_dim") and n <= eng.max_batch:
            eng(x, out=table[r0:r0 + n])
        else:                                    # the first batch: the block builds its engine for this frame size
            feat = net_backbone(x)
            feat = feat.reshape(n, -1).float()
            if table is None:
                table = torch.empty((len(frames), feat.shape[1]), dtype=torch.float32, device=feat.device)
            table[r0:r0 + n] = feat
            shape = tuple(x.shape[1:])
        r0 += n
    assert r0 == len(frames)
    return table


def evaluate_table(net, dataset, metrics, features=None, frames_idx=None, batch_size=64, num_workers=0, metric_batch=65536,
                   return_tams=False, keep=None):
    """``evaluate_windows`` through a row table (``TennisSet.window_table`` + ``net.forward_table``): any ``every``, ``stride``,
    ``padding`` and split layout the loader route accepts, in feature mode and on frames.  ``frames_idx``: ``(frames, idx)`` of
    ``dataset.window_table()`` if the caller has it.  ``features``: the (len(frames), F) table; None: in feature mode it is loaded
    with ``load_feature_table`` (every ``.npy`` once), on frames it is built by ``encode_table`` from the model's own backbone
    (``net.td.model``: every distinct frame decoded and encoded once, in batches of ``batch_size``).  Same return values and metric
    updates as ``evaluate_windows``, ``return_tams`` included."""
    frames, idx = dataset.window_table() if frames_idx is None else frames_idx
    if features is None:
        if getattr(net, "feats", False):
            features = load_feature_table(dataset, frames)
        else:
            features = encode_table(net.td.model, dataset, frames, batch_size, num_workers)
    if len(features) != len(frames):
        raise ValueError(f"evaluate_table: {len(features)} feature rows for a table of {len(frames)} frames")
    outputs = net.forward_table(features, idx, row_videos=[v for v, _ in frames], return_tam=return_tams)
    if return_tams:
        outputs, tam = outputs
    _keep_logits(keep, outputs, range(len(dataset)))
    labels = torch.tensor([dataset.classes.index(s[2]) for s in dataset._samples], dtype=torch.float32, device=outputs.device)
    for a in range(0, len(dataset), metric_batch):
        for metric in metrics:
            metric.update([labels[a:a + metric_batch]], [outputs[a:a + metric_batch]])
    out = outputs.cpu().numpy()
    results, ground_truths = dict(), dict()
    for i, sample in enumerate(dataset._samples):
        img_path = dataset.get_image_path(dataset._frames_dir, sample[0], sample[1])
        results[img_path] = out[i]
        ground_truths[img_path] = dataset.classes.index(sample[2])
    if return_tams:
        return results, ground_truths, tam_columns(net, dataset, range(len(dataset)), outputs, tam)
    return results, ground_truths


def check_dense_windows(flags):
    """What ``--dense_windows`` runs for these flags: "windows" (``evaluate_windows`` on stored features, with ``evaluate_table`` where
    the split has no ``window_rows`` form), "frames" (``evaluate_table`` on frames, each distinct frame encoded once), or None
    without the flag (and with ``--corpus_frames``, which has a route of its own).  Exits with the reason for what is still refused."""
    if not flags.dense_windows or flags.corpus_frames > 0:
        return None
    if flags.window <= 1 or flags.temp_pool not in ("gru", "lstm", "mean", "max"):
        raise SystemExit("--dense_windows needs --window W (> 1) and --temp_pool gru|lstm|mean|max")
    return "frames" if flags.feats_model is None else "windows"


def corpus_window_head(full, window, temp_pool, classes, stride=1, hidden=128):
    """``--corpus_frames N --dense_windows``: the temporal head over the gathered (N, F) matrix as ONE sequence (lo = 0,
    hi = N-1), one window per frame -> (logits, seconds of device work)."""
    n = full.shape[0]
    if temp_pool in ("gru", "lstm"):
        model = CNNRNN(None, num_classes=classes, type=temp_pool, hidden_size=hidden)
    elif temp_pool in ("mean", "max"):
        model = TemporalPooling(None, num_classes=classes, pool=temp_pool, feats=True)
    else:
        raise AssertionError("--dense_windows needs --temp_pool gru, lstm, mean or max")
    model.initialize()
    centre = torch.arange(n, dtype=torch.int32, device=full.device)
    lo, hi = torch.zeros_like(centre), torch.full_like(centre, n - 1)
    model.forward_windows(full, centre, lo, hi, window, stride, max_rows=n)      # builds the handles and their workspaces (untimed)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(full.device)
    t0.record()
    logits = model.forward_windows(full, centre, lo, hi, window, stride, max_rows=n)      # (one sequence: nowhere to cut)
    t1.record()
    torch.cuda.synchronize(full.device)
    return logits, t0.elapsed_time(t1) / 1e3


class NpyWriter:
    """The ``.npy`` side of ``--save_feats``: ``tn_npy_writer_*`` (csrc/npy_host.hip), a pool of host threads behind the C ABI that
    writes one NumPy-format-1.0 float32 file per feature row, byte for byte what ``np.save(path, row)`` writes, creating the
    directories and skipping files that exist (reference evaluate.py:312-316).  ``submit`` returns as soon as the rows are copied:
    the files of batch i are written while the GPU encodes batch i + 1 (the reference's np.save loop costs 13 ms of Python per 256
    frames against 1.8 ms of GPU time for their features)."""

    def __init__(self, threads: int | None = None):
        import ctypes as C
        from . import _lib
        self._C, self._lib = C, _lib
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.tn_npy_writer_create(int(threads or min(16, os.cpu_count() or 4)), C.byref(h)), "tn_npy_writer_create")
        self.handle = h
        self._written = self._skipped = 0

    def submit(self, rows: np.ndarray, paths, skip_existing: bool = True):
        C = self._C
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.ndim == 2 and rows.shape[0] == len(paths)
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        self._lib.check(self.lib.tn_npy_writer_submit(self.handle, rows.ctypes.data_as(C.c_void_p), rows.shape[0], rows.shape[1], arr,
                                                      1 if skip_existing else 0), "tn_npy_writer_submit")

    @staticmethod
    def sweep_stale(root: str, older_than_s: float = 600.0) -> int:
        """A run that is killed mid-write leaves ``<frame>.npy.tmp.<pid>.<thread>`` files behind (never a truncated ``.npy``:
        files are published by link / rename of a finished temporary).  Removes those under ``root`` that nobody has touched for
        ``older_than_s`` seconds (a live writer's temporaries are younger); -> the number removed.  Called by ``save_features`` on
        the feature directory before it writes."""
        import time
        n, now = 0, time.time()
        for d, _dirs, files in os.walk(root):
            for f in files:
                if ".npy.tmp." in f:
                    p = os.path.join(d, f)
                    try:
                        if now - os.path.getmtime(p) > older_than_s:
                            os.unlink(p)
                            n += 1
                    except OSError:
                        pass
        return n

    def drain(self):
        """waits for everything submitted; -> (files written, files skipped) since the last drain"""
        C = self._C
        w, s = C.c_int64(), C.c_int64()
        self._lib.check(self.lib.tn_npy_writer_drain(self.handle, C.byref(w), C.byref(s)), "tn_npy_writer_drain")
        out = (w.value - self._written, s.value - self._skipped)
        self._written, self._skipped = w.value, s.value
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.tn_npy_writer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def save_features(net, loader, dataset, ctx=None, verbose=True):
    """Reference evaluate.py:306-321: feat = net.backbone(x); one float32 ``.npy`` per
    frame at save_feature_path(idx), skipped when the file already exists.  The files are written by ``NpyWriter``'s threads
    behind the next batch's encode (round 4); the count returned is the number of files that did not exist."""
    writer = NpyWriter()
    if os.path.isdir(getattr(dataset, "feat_dir", "") or ""):
        NpyWriter.sweep_stale(dataset.feat_dir)
    pending = None          # (features on the device, paths) of the batch before: copied to the host and handed to the writer
                            # AFTER the next batch's forward has been queued, so that the copy waits for nothing but its own batch

    def flush(item):
        feat, paths = item
        if verbose:
            for feat_path in paths:
                if not os.path.exists(feat_path):
                    print("Saving %s" % feat_path)
        writer.submit(feat.cpu().numpy(), paths)

    try:
        for data, _labels, idxs in loader:
            feat = net.backbone(data)
            if pending is not None:
                flush(pending)
            pending = (feat, [dataset.save_feature_path(int(j)) for j in idxs])
        if pending is not None:
            flush(pending)
        written, _skipped = writer.drain()
    finally:
        writer.close()
    return written


def _backbone_dim(net, loader):
    """Feature width F of ``net.backbone`` (1024 at 224x224, 4096 at 512x512): asked of the engine when it exists,
    else measured on the first sample."""
    eng = getattr(net.backbone, "_engine", None)
    if eng is not None and hasattr(eng, "feature_dim"):
        return int(eng.feature_dim)
    data, _, _ = loader.collate([0])
    return int(net.backbone(data).shape[-1])


def save_features_sharded(net, loader, dataset, device=None, rank=None, world=None, group=None, block=1, verbose=False,
                          write=True, stats=None):
    """``save_features`` (evaluate.py:306-321) for N ranks: rank r encodes the batches ``sharding.rank_batches`` gives
    it (dataset order, no shuffle), writes their ``.npy`` files (skip-if-exists, as the reference) and the rows are
    all-gathered round by round behind the compute.  Returns (features (len(dataset), F) in dataset order — identical
    on every rank —, files written by this rank)."""
    if rank is None or world is None:
        rank, world = sharding._rank(group), sharding._world(group)
    fdim = _backbone_dim(net, loader)
    writer = NpyWriter() if write else None
    pending = []            # the batch before this one: written out once this one's forward is queued (see save_features)

    def flush():
        while pending:
            feat, paths = pending.pop(0)
            if verbose:
                for feat_path in paths:
                    if not os.path.exists(feat_path):
                        print("Saving %s" % feat_path)
            writer.submit(feat.detach().cpu().numpy(), paths)

    def encode(s, e):
        data, _labels, idxs = loader.collate(range(s, e))
        feat = net.backbone(data)
        if write:
            flush()
            pending.append((feat, [dataset.save_feature_path(int(j)) for j in idxs]))
        return feat
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    comm = sharding.feature_comm(device, group) if world > 1 else None
    try:
        full = sharding.extract_features_sharded(encode, len(dataset), loader.batch_size, fdim, device, rank=rank, world=world,
                                                 group=group, block=block, stats=stats, comm=comm)
        if writer is not None:
            flush()
        written = writer.drain()[0] if writer is not None else 0
    finally:
        if writer is not None:
            writer.close()
    return full, written


class SyntheticCorpus:
    """A corpus of ``n_frames`` synthetic decoded frames generated ON the device batch by batch (uint8 NHWC, seeded by
    the global frame index range, so every rank produces the same frame for the same index): stands in for the
    786 455 frames of the 5-match corpus, which cannot be shipped."""

    def __init__(self, n_frames, size, device, seed=1234):
        self.n, self.size, self.device, self.seed = int(n_frames), int(size), device, seed

    def __len__(self):
        return self.n

    def frames(self, s, e):
        g = torch.Generator(device=self.device)
        g.manual_seed(self.seed + s)
        return torch.randint(0, 256, (e - s, self.size, self.size, 3), generator=g, device=self.device, dtype=torch.uint8)


def extract_corpus(backbone, n_frames, batch, size, device, rank, world, block=4, seed=1234, reuse_frames=False):
    """BASELINE config C4: feature-extract over an ``n_frames`` corpus sharded over the ranks with the RCCL all-gather
    of the rows (chunked: one collective per round of ``block`` batches per rank, in flight behind the next round).
    Every batch of frames is generated on the device from its frame indices inside the loop (the result is then the
    same for any number of ranks: the checksum of the gathered matrix is a parity check); ``reuse_frames`` generates
    a rank's first batch once and re-uses it (frame synthesis is not part of the path).
    -> (features (n_frames, F) on every rank, dict of timings)."""
    corpus = SyntheticCorpus(n_frames, size, device, seed)
    cached = {}

    def encode_input(s, e):
        if reuse_frames:
            if (e - s) not in cached:
                cached[e - s] = corpus.frames(s, e)
            return cached[e - s]
        return corpus.frames(s, e)

    def encode(s, e):
        return backbone(encode_input(s, e))
    fdim = int(backbone(corpus.frames(0, min(batch, n_frames))).shape[-1])      # also builds the engine (untimed)
    # the HIP encoder runs consecutive batches pipelined (its two half-batch streams are joined once per gather round, not
    # in every forward); a batch's frames stay referenced until that join
    eng = getattr(backbone, "_engine", None)
    pipelined = eng is not None and hasattr(eng, "set_pipelined") and device.type == "cuda"
    live = []

    def encode_into(s, e, rows):
        x = encode_input(s, e)
        if x.shape[0] <= eng.max_batch:
            live.append(x)
            eng(x, out=rows)
        else:
            rows.copy_(backbone(x))

    def join():
        eng.join(0)
        eng.join(1)
        live.clear()
    fence = (lambda: (torch.distributed.barrier() if world > 1 else None, torch.cuda.synchronize() if device.type == "cuda" else None))
    comm = sharding.feature_comm(device) if world > 1 else None
    stats = {}
    fence()
    t0 = time.perf_counter()
    if pipelined:
        eng.set_pipelined(True)
    try:
        full = sharding.extract_features_sharded(encode, n_frames, batch, fdim, device, rank=rank, world=world, block=block, stats=stats,
                                                 encode_into=encode_into if pipelined else None, join=join if pipelined else None,
                                                 comm=comm)
    finally:
        if pipelined:
            eng.set_pipelined(False)
    fence()
    dt = time.perf_counter() - t0
    stats.update(seconds=dt, frames_per_sec=n_frames / dt, feature_dim=fdim,
                 gather_GBps_per_rank=(stats["gather_bytes_per_rank"] * max(world - 1, 0) / dt / 1e9))
    if device.type == "cuda":        # HBM in use on this rank's device when the corpus is done (everything: the library's workspace, torch's pool, the feature matrix)
        free_b, total_b = torch.cuda.mem_get_info(device)
        stats.update(hbm_used_GB=(total_b - free_b) / 1e9, hbm_total_GB=total_b / 1e9)
    return full, stats


def best_or_newest_params(mod_path, need_scores):
    """The parameter file the reference would load (evaluate.py:186-200,206-212,223-240): epoch with the best
    ``scores.txt`` line; without a scores file the newest ``NNNN.params`` (None when the directory holds neither and
    ``need_scores`` is False)."""
    from .train import best_epoch_from_scores, newest_params
    scores = os.path.join(mod_path, "scores.txt")
    if os.path.exists(scores):
        ep, sc = best_epoch_from_scores(scores)
        if ep >= 0:
            print("Testing best model from Epoch %d with score of %f" % (ep, sc))
            return os.path.join(mod_path, "{:04d}.params".format(ep))
    if need_scores and not os.path.isdir(mod_path):
        return None
    return newest_params(mod_path)


def build_parser():
    p = argparse.ArgumentParser(description="tennis_amd evaluate (flags of reference evaluate.py:30-75)")
    p.add_argument("--backbone", default="DenseNet121")
    p.add_argument("--fp16_conversion", default="nearest", choices=["nearest", "calibrated", "exact", "fp32", "fp32x3"],
                   help="how the checkpoint's fp32 conv weights become the fp16 model (not a reference flag): plain rounding, "
                        "rounding calibrated on the library's built-in calibration frames (the same model on every rank; features within "
                        "1e-3 of the fp32 evaluation on natural content at full speed, DESIGN.md), hi + lo weight pairs (twice the "
                        "MFMAs), fp32: no conversion, the network evaluated in fp32 (the fp32 evaluation of any checkpoint within "
                        "1e-3, at the f32 matrix rate), or fp32x3: that fp32 network with every operand as three bf16 terms on the "
                        "bf16 matrix pipe (the same bar, faster)")
    p.add_argument("--model_id", default="0000")
    p.add_argument("--split_id", default="02")
    p.add_argument("--split", default="test")
    p.add_argument("--data_shape", type=int, default=224)
    p.add_argument("--every", default="1, 1, 1")
    p.add_argument("--window", type=int, default=1)
    p.add_argument("--padding", type=int, default=1)
    p.add_argument("--stride", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--num_gpus", type=int, default=1)
    p.add_argument("--save_feats", action="store_true")
    p.add_argument("--feats_model", default=None)
    p.add_argument("--temp_pool", default=None, help="mean, max, gru or lstm")
    # the rest of the reference's flags (evaluate.py:30-75), so that its documented command lines parse unchanged, e.g.
    # `python evaluate.py --model_id 0042 --backbone DenseNet121 --temp_pool gru --window 30 --backbone_from_id 0006 --feats_model 0006
    # --freeze_backbone` (models/README.md:58)
    p.add_argument("--backbone_from_id", default=None,
                   help="load the frame model's parameters from the newest .params of this model id before the temporal model is put around it (evaluate.py:142-151)")
    p.add_argument("--freeze_backbone", action="store_true", help="accepted (evaluate.py:153-155 sets grad_req = 'null': nothing to do without gradients)")
    p.add_argument("--balance", default="True, False, False", help="accepted; the test set is never balanced (evaluate.py:109)")
    p.add_argument("--vis", action="store_true", help="visualisation output is outside the accelerated path (SURVEY 2a): refused")
    p.add_argument("--flow", default="", help="optical-flow input is outside the accelerated path (SURVEY 2a): anything but '' is refused")
    p.add_argument("--root", default="data")
    p.add_argument("--num_workers", type=int, default=3,
                   help="loader threads (reference: DataLoader worker processes, evaluate.py:113); on the device-decode route each owns a JPEG decoder on its own stream")
    p.add_argument("--decode", default="device", choices=["device", "host", "auto"],
                   help="where on-disk JPEG frames are decoded: on the GPU (tennis_amd.image), on the host (Pillow), or device with a host fallback for files the device decoder refuses")
    p.add_argument("--frames_per_video", type=int, default=16)
    p.add_argument("--exp_root", default=os.path.join("models", "vision", "experiments"))
    p.add_argument("--corpus_frames", type=int, default=0,
                   help="config C4: encode a synthetic corpus of this many frames sharded over --num_gpus ranks with "
                        "the all-gather of the feature rows (786455 = the 5-match corpus); prints one JSON line")
    p.add_argument("--gather_block", type=int, default=4, help="batches per rank per all-gather round")
    p.add_argument("--corpus_reuse_frames", action="store_true", help="C4: generate one synthetic batch per rank and re-use it")
    p.add_argument("--dense_windows", action="store_true",
                   help="dense windowed evaluation (not a reference flag): with --window W --temp_pool gru|lstm|mean|max every frame is "
                        "read once and projected once, the windows are gathered on the GPU - with --feats_model M from the stored "
                        "features (evaluate_windows; evaluate_table for splits without an arithmetic window form), without it from "
                        "frames, each distinct frame decoded and encoded once (evaluate_table); with --corpus_frames N the head "
                        "runs over the gathered matrix as one sequence")
    p.add_argument("--save_cams", action="store_true",
                   help="frame model only (--window 1, no --feats_model, no --temp_pool; not a reference flag): also write "
                        "<split>_cams.npz into the experiment's directory - per frame the class activation map of its arg-max class "
                        "(7 x 7 cells at 224, 14 x 14 at 512), the class, the label, that class's logit, the video and the frame "
                        "number (evaluate.load_cams reads it); the maps come out of the same forward, the metrics do not change")
    p.add_argument("--save_tams", action="store_true",
                   help="windowed model that ends in max over the window -> Dense (--window W > 1 with --temp_pool gru|lstm|max, with or "
                        "without --feats_model / --dense_windows, one rank; not a reference flag): also write <split>_tams.npz into the "
                        "experiment's directory - per sample the temporal activation map of its arg-max class (one number per window "
                        "step; with that class's Dense bias they sum to its logit), the class, the label, the logit, the bias, the "
                        "video, the centre frame and the frame number every window step read (evaluate.load_tams reads it).  A map "
                        "names the step whose state the logit was read from - a recurrent state has seen the steps before it - not "
                        "a single frame that caused it.  The maps come out of the same forward, the metrics do not change")
    p.add_argument("--save_events", action="store_true",
                   help="also decode the per-sample logits into events on the GPU (every route that yields them: the frame model, windowed "
                        "models on the loader route, --dense_windows on stored features and on frames; one rank; not a reference flag) "
                        "and write <split>_events.npz into the experiment's directory - per predicted event the video, first and last "
                        "frame, class, mean and peak score, per ground-truth event (runs of one label in time order) the same without "
                        "scores, and event precision / recall / F1 at tIoU 0.1, 0.3, 0.5 (events.load_events reads it).  A run of the "
                        "background class is an event too.  The per-frame scores and results do not change")
    p.add_argument("--event_smooth", type=int, default=None,
                   help="with --save_events: odd width in [1, 63] of the window the class probabilities are averaged over before the "
                        "arg-max (cut at video boundaries; default 1, no smoothing).  Moves event boundaries by up to (width - 1) / 2 frames")
    p.add_argument("--event_switch_cost", type=float, default=None,
                   help="with --save_events, instead of smoothing: decode every video as one label path that maximises the summed "
                        "per-frame scores (logit minus the frame's largest logit) minus this penalty for every change of label "
                        "(Viterbi on the GPU; finite, >= 0, in logit units; 0 is the per-frame arg-max).  A one-frame glitch that leads "
                        "by less than twice the penalty is absorbed, boundaries stay where the scores put them.  For a stay "
                        "probability s over C classes: ln(s (C - 1) / (1 - s)).  Not together with --event_smooth above 1")
    p.add_argument("--event_transitions", type=str, default=None, metavar="train|FILE.npy",
                   help="with --save_events, instead of smoothing or one switch cost: decode every video as one label path under a "
                        "(classes, classes) matrix of transition scores, entry [from, to] added where a frame labelled `from` is "
                        "followed by one labelled `to` (an HMM over the frame classifier, Viterbi on the GPU).  train: the log "
                        "probabilities of the label bigrams of this run's train split, counted in time order with the test split's "
                        "--every, --window, --stride and --padding, unbalanced (labels only: nothing is encoded).  FILE.npy: a matrix "
                        "of your own, every entry <= 0, -inf off the diagonal forbids a transition.  Not together with "
                        "--event_smooth above 1 or --event_switch_cost")
    p.add_argument("--event_transition_prior", type=float, default=None,
                   help="with --event_transitions train: the count added to every bigram before the logarithm (> 0; default 1)")
    p.add_argument("--event_transition_scale", type=float, default=None,
                   help="with --event_transitions train: the factor on the log probabilities, i.e. how much the grammar weighs "
                        "against the per-frame scores (> 0; default 1)")
    p.add_argument("--event_posteriors", action="store_true",
                   help="with --save_events and --event_transitions or --event_switch_cost: score every event with the posterior "
                        "probability of its class under the same model (forward-backward on the GPU) - per frame the probability of "
                        "the path's label given ALL frames of the video, its mean and maximum over the event - in place of the "
                        "frame's own softmax probability.  The events themselves do not change")
    return p


def event_transitions(flags, test_set, every):
    """The matrix of ``--event_transitions`` -> ``(T (classes, classes) float32, where it came from)``.  ``train``: the bigrams of the
    run's own train split in time order (``events.transition_scores``); the split is built for its labels only."""
    from .events import check_transitions, time_order, transition_scores
    classes = len(test_set.classes)
    if flags.event_transitions != "train":
        return check_transitions(np.load(flags.event_transitions, allow_pickle=False), classes, "--event_transitions"), flags.event_transitions
    train_set = TennisSet(root=flags.root, split="train", every=every, padding=flags.padding, stride=flags.stride, window=flags.window,
                          model_id=flags.model_id, split_id=flags.split_id, balance=False, data_shape=flags.data_shape,
                          frames_per_video=flags.frames_per_video, decode=flags.decode)
    rows, start, _, _ = time_order(train_set)
    labels = np.asarray([train_set.classes.index(train_set._samples[int(i)][2]) for i in rows], np.int64)
    prior = 1.0 if getattr(flags, "event_transition_prior", None) is None else flags.event_transition_prior
    scale = 1.0 if getattr(flags, "event_transition_scale", None) is None else flags.event_transition_scale
    return (transition_scores(labels, start, classes, prior=prior, scale=scale),
            "the %d label bigrams of the train split (prior %g, scale %g)" % (int((start == 0).sum()), prior, scale))


def main(argv=None):
    flags = build_parser().parse_args(argv)
    check_save_cams(flags)                                                  # refusals before any device work
    check_save_tams(flags)
    check_save_events(flags)
    if flags.num_gpus > 1 and not sharding.under_launcher():
        # evaluate.py:101-102 builds ctx = [gpu(0) .. gpu(N-1)] in one process; here: one process per GPU
        if torch.cuda.is_available() and flags.num_gpus > torch.cuda.device_count():
            raise SystemExit(f"--num_gpus {flags.num_gpus} but only {torch.cuda.device_count()} GPUs are visible")
        sharding.launch(main, flags.num_gpus, (list(sys.argv[1:] if argv is None else argv),))
        return 0
    rank, world, dev = sharding.init_distributed()
    try:
        rc = _main_rank(flags, rank, world, dev)
        if world > 1 and torch.distributed.is_initialized():
            torch.distributed.barrier()          # success path only: a rank that raised must not park the others' collectives
        return rc
    finally:
        if world > 1 and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def _main_rank(flags, rank, world, dev):
    if flags.flow or flags.vis:
        raise NotImplementedError("--flow / --vis: optical-flow input and visualisation are outside the accelerated path (SURVEY 2a)")
    if flags.num_workers < 0:                                               # the reference's -1 = cpu_count() (evaluate.py:80-81)
        flags.num_workers = 3                                               # (files -> features peaks at three decoder threads: scripts/bench_pipeline.py, profiles/r05_c_*)
    every = [int(s) for s in flags.every.split(",")]
    check_dense_windows(flags)                                              # refusals before anything is built
    check_save_cams(flags, world)
    check_save_tams(flags, world)
    check_save_events(flags, world)
    flags.save_tams = getattr(flags, "save_tams", False)                    # (flags built by hand, without the newer switches)
    flags.save_events = getattr(flags, "save_events", False)
    if flags.corpus_frames > 0:                                            # BASELINE config C4
        backbone = get_model(flags.backbone, pretrained=True, max_batch=flags.batch_size, conversion=flags.fp16_conversion).features
        full, st = extract_corpus(backbone, flags.corpus_frames, flags.batch_size, flags.data_shape, dev, rank, world,
                                  block=flags.gather_block, reuse_frames=flags.corpus_reuse_frames)
        head = {}
        if flags.dense_windows:                                             # the temporal stage over the matrix every rank now holds
            logits, secs = corpus_window_head(full, flags.window, flags.temp_pool, len(TennisSet._get_classes(flags.root)), flags.stride)
            head = {"window": flags.window, "temp_pool": flags.temp_pool, "head_seconds": round(secs, 4),
                    "samples_per_sec": round(flags.corpus_frames / secs, 1), "logits_checksum": float(logits.double().sum().item())}
        if rank == 0:
            print(json.dumps({**head, "config": "C4 corpus feature-extract + all-gather", "frames": flags.corpus_frames,
                              "n_gpus": world, "batch": flags.batch_size, "rounds": st["rounds"],
                              "frames_per_sec": round(st["frames_per_sec"], 1), "seconds": round(st["seconds"], 3),
                              "feature_matrix_MB": round(full.numel() * 4 / 1e6, 1),
                              "gather_GBps_per_rank": round(st["gather_GBps_per_rank"], 3),
                              "hbm_used_GB": round(st.get("hbm_used_GB", 0.0), 2), "hbm_total_GB": round(st.get("hbm_total_GB", 0.0), 1),
                              "checksum": float(full.double().sum().item())}))
        return 0
    # evaluate.py:91-98: Resize(s + 32) / CenterCrop(s) / ToTensor / Normalize, here one GPU launch per batch; the
    # synthetic source already produces data_shape frames, so only data on disk goes through it
    transform_test = None
    if flags.feats_model is None and os.path.exists(os.path.join(flags.root, "splits", flags.split_id, flags.split + ".txt")):
        transform_test = transforms.Compose([transforms.Resize(flags.data_shape + 32),
                                             transforms.CenterCrop(flags.data_shape),
                                             transforms.ToTensor(),
                                             transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    test_set = TennisSet(root=flags.root, transform=transform_test, split=flags.split, every=every[2], padding=flags.padding,
                         stride=flags.stride, window=flags.window, model_id=flags.model_id,
                         split_id=flags.split_id, balance=False, feats_model=flags.feats_model,
                         save_feats=flags.save_feats, data_shape=flags.data_shape,
                         frames_per_video=flags.frames_per_video, decode=flags.decode)
    test_data = DataLoader(test_set, batch_size=flags.batch_size, shuffle=False, num_workers=flags.num_workers)

    model = None
    if flags.feats_model is None:                                           # evaluate.py:118-135
        backbone_net = get_model(flags.backbone, pretrained=True, conversion=flags.fp16_conversion).features
        model = FrameModel(backbone_net, len(test_set.classes))
    elif flags.temp_pool in ["max", "mean"]:                                # evaluate.py:136-138
        backbone_net = get_model(flags.backbone, pretrained=True, conversion=flags.fp16_conversion).features
        model = FrameModel(backbone_net, len(test_set.classes))
    if flags.window > 1:                                                    # evaluate.py:139-162
        if flags.backbone_from_id and model is not None:                    # evaluate.py:142-151
            bb_dir = os.path.join(flags.exp_root, flags.backbone_from_id)
            if os.path.isdir(bb_dir):
                files = sorted((f for f in os.listdir(bb_dir) if f.endswith(".params")), reverse=True)
                if files:
                    model.initialize()
                    model.load_parameters(os.path.join(bb_dir, files[0]))
                    print("Loaded backbone params: {}".format(os.path.join(bb_dir, files[0])))
        if flags.temp_pool in ["gru", "lstm"]:
            model = CNNRNN(model, num_classes=len(test_set.classes), type=flags.temp_pool, hidden_size=128)
        elif flags.temp_pool not in ["mean", "max"]:
            raise AssertionError("window > 1 needs --temp_pool (the 3-D rdnet backbone is out of scope)")
    model.initialize()
    model.hybridize()

    # trained parameters: the best epoch of scores.txt (evaluate.py:186-200,223-240), else the newest NNNN.params
    # (:206-212); an experiment directory without either leaves the (seeded) initial parameters, with a notice
    mod_path = os.path.join(flags.exp_root, flags.model_id)
    if flags.temp_pool in ["max", "mean"] and flags.feats_model is not None and not flags.save_feats:
        mod_path = os.path.join(flags.exp_root, flags.feats_model)          # evaluate.py:219-222
    params_file = best_or_newest_params(mod_path, need_scores=False)
    if params_file is not None:
        model.load_parameters(params_file)
        print("Loaded model params: {}".format(params_file))
    elif rank == 0:
        print("no trained parameters under %s: evaluating the initial parameters" % mod_path)

    if flags.save_feats:                                                    # evaluate.py:186-204
        # one code path for any number of ranks (world 1: no collective, the shard IS the matrix)
        full, n = save_features_sharded(model, test_data, test_set, device=dev, rank=rank, world=world,
                                        block=flags.gather_block, verbose=(world == 1))
        print("[rank %d of %d] wrote %d feature files under %s; feature matrix %s on every rank" %
              (rank, world, n, test_set.feat_dir, tuple(full.shape)))
        return 0

    if flags.temp_pool in ["max", "mean"]:                                  # evaluate.py:242-244
        model = TemporalPooling(model, pool=flags.temp_pool, num_classes=0, feats=flags.feats_model is not None)
    test_metrics = [PRF1(label_names=test_set.classes)]
    tic = time.time()
    tams = {"return_tams": True} if flags.save_tams else {}                 # (a call without the flag is the call it was)
    cols = None
    kept = {} if flags.save_events else None                                # (None: every call below is the call it was)
    keep = {} if kept is None else {"keep": kept}
    tams = dict(tams, **keep)
    if flags.dense_windows:
        route = check_dense_windows(flags)
        if rank != 0:                                                       # one pass over one matrix: nothing to shard
            return 0
        if route == "frames":
            results, gts, *cols = evaluate_table(model, test_set, test_metrics, batch_size=flags.batch_size,
                                                 num_workers=flags.num_workers, **tams)
        else:
            try:
                test_set.window_rows()
            except ValueError as e:
                print("--dense_windows: this split has no (centre, lo, hi) window form (%s): evaluating through the row table" % e)
                route = "table"
            if route == "table":
                results, gts, *cols = evaluate_table(model, test_set, test_metrics, **tams)
            else:
                results, gts, *cols = evaluate_windows(model, test_set, test_metrics, **tams)
    elif world > 1:                                                           # each rank tests batches rank::world
        results, gts = evaluate_model(model, _RankBatches(test_data, rank, world), test_set, test_metrics)
        comm = sharding.feature_comm(dev)
        for m in test_metrics:                                              # confusion counts add up over the ranks
            packed = torch.from_numpy(np.concatenate([m.mat.ravel(), m.scores.ravel()])).to(dev)
            if comm is not None and packed.dtype in (torch.float32, torch.int64):
                comm.allreduce_(packed).wait()                              # tn_allreduce_* of the C-ABI
            else:
                torch.distributed.all_reduce(packed)
            packed = packed.cpu().numpy()
            m.mat = packed[:m.mat.size].reshape(m.mat.shape)
            m.scores = packed[m.mat.size:].reshape(m.scores.shape)
        if rank != 0:
            return 0
    elif flags.save_cams:
        results, gts, cols = evaluate_model_cams(model, test_data, test_set, test_metrics, **keep)
        cams_file = os.path.join(flags.exp_root, flags.model_id, flags.split + "_cams.npz")
        save_cams(cams_file, **cols)
        print("Saved %d class activation maps %s: %s" % (len(cols["cam"]), tuple(cols["cam"].shape[1:]), cams_file))
    elif flags.save_tams:
        results, gts, *cols = evaluate_model_tams(model, test_data, test_set, test_metrics, **keep)
    else:
        results, gts = evaluate_model(model, test_data, test_set, test_metrics, **keep)
    if flags.save_tams:
        tams_file = os.path.join(flags.exp_root, flags.model_id, flags.split + "_tams.npz")
        save_tams(tams_file, **cols[0])
        print("Saved %d temporal activation maps of %d steps: %s" % (len(cols[0]["tam"]), cols[0]["tam"].shape[1], tams_file))
    if kept is not None:                                                     # the logits never left the device: decode them there
        cost = getattr(flags, "event_switch_cost", None)
        path = {} if cost is None else {"switch_cost": cost}                 # (without the flag the call is the call it was)
        if getattr(flags, "event_transitions", None) is not None:
            matrix, source = event_transitions(flags, test_set, every[2])
            off = matrix[~np.eye(len(matrix), dtype=bool)]
            print("Event transitions (%d x %d) from %s: smallest diagonal entry %.4g, largest off-diagonal entry %.4g" %
                  (matrix.shape[0], matrix.shape[1], source, np.diagonal(matrix).min(), off.max() if off.size else float("nan")))
            path["transitions"] = matrix
        if getattr(flags, "event_posteriors", False):
            path["posteriors"] = True
        ev_cols, ev_metric = decode_split(test_set, torch.cat(kept["logits"]), kept["order"], smooth=getattr(flags, "event_smooth", None) or 1,
                                          **path)
        events_file = os.path.join(flags.exp_root, flags.model_id, flags.split + "_events.npz")
        save_events(events_file, **ev_cols)
        print(event_table(ev_cols, test_set.classes))
        print("[Events] " + ", ".join("{}={:.3f}".format(k, v) for k, v in ev_metric.get() if k.startswith("AVG_")))
        print("Saved %d events (%d ground truth): %s" % (len(ev_cols["video"]), len(ev_cols["gt_video"]), events_file))
    str_ = "Test set:"                                                       # evaluate.py:250-255
    for i in range(len(test_set.classes)):
        str_ += "\n"
        for j in range(len(test_set.classes)):
            str_ += str(test_metrics[0].mat[i, j]) + "\t"
    print(str_)
    str_ = "[Finished] "
    for res in test_metrics[0].get():
        str_ += ", Test_{}={:.3f}".format(res[0], res[1])
    str_ += "  # Samples: {}, Time Taken: {:.1f}".format(len(test_set), time.time() - tic)
    print(str_)
    return 0


class _RankBatches:
    """The batches b with b mod world == rank of a loader (dataset order)."""

    def __init__(self, loader, rank, world):
        self.loader, self.rank, self.world = loader, rank, world

    def __iter__(self):
        # batch ids are filtered BEFORE collation where the loader allows it (tennis_amd.dataset.DataLoader.batches_of): a
        # rank then reads, decodes and resizes only its own batches
        if hasattr(self.loader, "batches_of"):
            yield from self.loader.batches_of(self.rank, self.world)
            return
        for b, batch in enumerate(self.loader):
            if b % self.world == self.rank:
                yield batch


if __name__ == "__main__":
    raise SystemExit(main())
