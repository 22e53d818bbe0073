"""Caption-mode dataset, batching and the captioning evaluate() driver — mirrors of the
caption branch of reference dataset.py::TennisSet (dataset.py:52-74,154-183,235-247),
utils/captioning.py::get_dataloaders/write_sentences (:28-95) and
train_gnmt.py::evaluate (:264-302).  Two sources: ON DISK when ``root`` holds the reference's layout
(``splits/<split_id>/<split>.txt``, ``annotations/points.txt`` + ``captions.txt``, per-frame ``.npy`` features under
``features/<feats_model>/`` as ``evaluate --save_feats`` writes them; parsed by ``TennisSet.load_data``), else SYNTHETIC
(the TenniSet features and captions are not available).  Either source yields FEATURES (``feats_model``, dataset.py:42-44,
169-171) or, without ``feats_model``, the point's FRAMES (dataset.py:172-176: frame mode, the CNN inside the captioner) through
``TennisSet``'s frame reading and ``transform``.

One sample = one *point*: every `every`-th frame feature in [start, end), stacked (T,F), plus
the caption ids ``[<bos>] + vocab[tokens][:max_cap_len] + [<eos>]`` as int32 (dataset.py:67-73);
val/test reuse the train vocab (train_gnmt.py:200-203).  Batches are zero-padded like
``gluonnlp.data.batchify.Pad()`` (target padding is id 0), lengths are float32.
"""
from __future__ import annotations

import io
import math
import zlib

import numpy as np
import torch

from .models.captioning.gnmt import Vocab

WORDS = ("the near far player serves hits a forehand backhand return volley into net in out left right "
         "middle ball wide deep cross court down line fault ace winner long short lob smash second first").split()


class CaptionSet:
    """``TennisSet(captions=True, ...)`` counterpart.  The source is chosen by its arguments: ``feats_model`` -> (T, F) features;
    ``frames=True`` -> the point's frames; neither, on disk -> ``ValueError`` (``TennisSet(captions=True, ...)`` passes ``frames="auto"``,
    which is frames exactly where the reference reads frames: on disk without ``feats_model``, dataset.py:172-176).
    Frame items are (T, 3, S, S) fp32 after a per-frame ``transform`` (default: ToTensor
    + Normalize), or the decoded (T, H, W, 3) uint8 frames when the transform is ``device_batched`` (``tennis_amd.transforms.Compose``),
    which ``bucketed_batches`` then runs once per batch on the GPU."""

    def __init__(self, split="train", every=1, max_cap_len=-1, vocab=None, inference=False, n_points=24,
                 feature_dim=1024, mean_frames=40, seed=7, root=None, split_id="02", feats_model=None, frames=False,
                 transform=None, data_shape=224, decode="host"):
        self._captions, self._split, self._every, self._inference = True, split, every, inference
        self._points, self._samples = {}, []
        self._feat_dir, self._frames, self._transform = None, None, None
        import os
        from .dataset import TennisSet
        on_disk = root is not None and os.path.exists(os.path.join(root, "splits", split_id, split + ".txt"))
        if frames == "auto":          # TennisSet(captions=True): frames where the reference reads frames, features where it reads features
            frames = on_disk and feats_model is None
        if on_disk:
            # dataset.py:35-52: the points of this split from annotations/points.txt + captions.txt; frames or their features
            if feats_model is None and not frames:
                raise ValueError("the caption source on disk reads pre-extracted features (feats_model, dataset.py:42-44) or the "
                                 "points' frames (frames=True; TennisSet(captions=True, ...) without feats_model selects them)")
            ts = TennisSet(root=root, split=split, split_id=split_id, every=1, balance=False, feats_model=feats_model,
                           transform=transform, decode=decode)
            for pid, pt in ts._points.items():
                self._points[pid] = [pt[0], int(pt[1]), int(pt[2]), 0, pt[-1]]
            self._samples = list(self._points.keys())
            if feats_model is not None:
                self._feat_dir, self._feat_path = ts.feat_dir, ts.get_feature_path
            else:
                self._frames, self._transform = ts, ts.transform
        else:
            if frames:        # distinct synthetic frames per (video, frame): TennisSet's synthetic frame source
                self._frames = TennisSet(transform=transform, data_shape=data_shape, frames_per_video=1, seed=seed, synthetic=True)
                self._transform = self._frames.transform
            rng = np.random.default_rng(zlib.crc32(f"{split}:{seed}".encode()))
            for i in range(n_points):
                start = int(rng.integers(0, 1000))
                n = int(np.clip(rng.normal(mean_frames, mean_frames / 3), 4, 3 * mean_frames))
                cap = " ".join(rng.choice(WORDS, size=int(rng.integers(4, 14))))
                pid = f"P{split}{i:04d}"
                self._points[pid] = ["V006", start, start + n, 0, cap]
                self._samples.append(pid)
        self._fdim, self._seed = feature_dim, seed
        if vocab is None:                                              # dataset.py:55-58
            counter = {}
            for p in self._points.values():
                for w in p[4].split():
                    counter[w] = counter.get(w, 0) + 1
            self.vocab = Vocab(counter)
        else:
            self.vocab = vocab
        for pid in self._samples:                                      # dataset.py:62-74
            toks = self._points[pid][4].split()
            ids = self.vocab[toks[:max_cap_len] if max_cap_len >= 0 else toks]
            ids = [self.vocab[self.vocab.bos_token]] + ids + [self.vocab[self.vocab.eos_token]]
            self._points[pid].append(np.array(ids, dtype=np.int32))

    def __len__(self):
        return len(self._samples)

    def get_captions(self, ids=False, split=False):                    # dataset.py:76-91
        caps = [self._points[s][5] if ids else self._points[s][4] for s in self._samples]
        return [c.split() for c in caps] if split and not ids else caps

    def _feature(self, vid, frame):
        if self._feat_dir is not None:                                  # dataset.py:169-171
            return np.load(self._feat_path(self._feat_dir, vid, frame)).astype(np.float32)
        s = zlib.crc32(f"{vid}:{frame}:{self._seed}".encode())
        return np.abs(np.random.default_rng(s).normal(0, 1, self._fdim)).astype(np.float32) * 0.5

    def __getitem__(self, idx):                                        # dataset.py:154-183
        point = self._points[self._samples[idx]]
        vid, start, end, cap = point[0], int(point[1]), int(point[2]), point[5]
        load = self._frames.load_frame if self._frames is not None else self._feature
        imgs = np.stack([load(vid, f) for c, f in enumerate(range(start, end)) if c % self._every == 0])
        if self._inference:
            return imgs, cap, len(imgs), len(cap), idx
        return imgs, cap, len(imgs), len(cap)

    def get_data_lens(self):                                           # dataset.py:235-247 (off by one kept)
        return [(int((int(self._points[s][2]) - int(self._points[s][1]) + 1) / self._every), len(self._points[s][5]))
                for s in self._samples]

    def get_clip_lens(self):
        """the exact number of frames item i stacks (``get_data_lens`` keeps the reference's rounding, which can fall one short)"""
        return [len(range(int(self._points[s][1]), int(self._points[s][2]), self._every)) for s in self._samples]


    def clip_frames(self, idx):
        """the (video, frame) pairs item ``idx`` stacks, in order (``every`` honoured) - ``__getitem__``'s own selection"""
        point = self._points[self._samples[idx]]
        return [(point[0], f) for f in range(int(point[1]), int(point[2]), self._every)]

    def clip_table(self):
        """-> (frames, idx, lens): the split as rows of one feature table, for training and evaluating from a device-resident table
        instead of the loader.  ``frames``: the sorted distinct (video, frame) pairs any point reads; ``idx`` (len(self), max clip
        length) int32: item i's step t is table row ``idx[i, t]``, -1 past the clip's length; ``lens`` = ``get_clip_lens()``.  Points may
        overlap, repeat or come in any order: a frame two points share is one row."""
        if self._frames is not None:
            raise ValueError("clip_table: the feature table serves feature mode; this set reads frames")
        clips = [self.clip_frames(i) for i in range(len(self))]
        frames = sorted({vf for c in clips for vf in c})
        row = {vf: r for r, vf in enumerate(frames)}
        lens = [len(c) for c in clips]
        idx = np.full((len(clips), max(lens, default=0)), -1, np.int32)
        for i, c in enumerate(clips):
            idx[i, :len(c)] = [row[vf] for vf in c]
        return frames, idx, lens


def load_clip_table(dataset, frames):
    """The (len(frames), F) float32 feature table of ``CaptionSet.clip_table``: row r is the feature of ``frames[r]`` = (video, frame)
    through the dataset's own ``_feature`` - the ``.npy`` under its feature directory, each read exactly once (the loader reads it once
    per point that holds it, every epoch), or the synthetic source's vector."""
    if not len(frames):
        raise ValueError("load_clip_table: no frames")
    from .evaluate import read_rows
    return read_rows(lambda r: dataset._feature(frames[r][0], frames[r][1]), len(frames))


def upload_clip_table(dataset):
    """-> (table on the GPU, idx): one split's features uploaded once (``--feats_on_device``).  Every rank of a data-parallel run holds
    the whole table; one that does not fit raises with its size - the loader route remains the answer there."""
    frames, idx, _ = dataset.clip_table()
    host = load_clip_table(dataset, frames)
    try:
        return torch.from_numpy(host).cuda(), idx
    except RuntimeError as e:           # torch.cuda.OutOfMemoryError is one
        raise RuntimeError("feats_on_device: the {} x {} float32 feature table ({:.1f} MiB) does not fit on the GPU; train without "
                           "the flag (the loader route)".format(host.shape[0], host.shape[1], host.nbytes / 2 ** 20)) from e


def pad_batchify(samples):
    """``btf.Tuple(Pad(), Pad(), Stack('float32'), Stack('float32')[, Stack()])`` (utils/captioning.py:33-37)."""
    tmax = max(s[0].shape[0] for s in samples)
    lmax = max(len(s[1]) for s in samples)
    src = np.zeros((len(samples), tmax) + samples[0][0].shape[1:], samples[0][0].dtype)      # (T, F) features or (T, ...) frames
    tgt = np.zeros((len(samples), lmax), np.int32)
    for i, s in enumerate(samples):
        src[i, :s[0].shape[0]] = s[0]
        tgt[i, :len(s[1])] = s[1]
    out = [src, tgt, np.array([s[2] for s in samples], np.float32), np.array([s[3] for s in samples], np.float32)]
    if len(samples[0]) > 4:
        out.append(np.array([s[4] for s in samples], np.int64))
    return tuple(out)


def bucketed_batches(dataset, batch_size, num_buckets=5, shuffle=False, seed=0, epoch=0, rank=0, world=1, rows=None):
    """Stand-in for ``FixedBucketSampler(lengths, batch_size, num_buckets, shuffle)`` with constant-width buckets:
    samples are grouped by target length so padding stays small; instance ids travel with the batch, evaluate()
    restores the dataset order.  ``shuffle=False`` is the reference's validation / test sampler
    (utils/captioning.py:62-86); ``shuffle=True`` its TRAINING sampler (:48-55): the samples of a bucket are permuted
    before they are cut into batches and the batches are visited in random order, afresh every epoch
    (``default_rng(seed + epoch)``).  ``rank`` / ``world``: a data-parallel rank takes batches rank::world of that
    (identically seeded) list, padded by wrapping so that every rank runs the same number of steps.
    ``rows``: ``CaptionSet.clip_table()``'s idx - the same batches, targets and lengths, but the source element is the batch's
    (B, longest clip of the batch) int32 table rows (-1 = padding) instead of the stacked features; no item is read, no file opened."""
    lens = [l[-1] for l in dataset.get_data_lens()]
    lo, hi = min(lens), max(lens)
    width = max(1, math.ceil((hi - lo + 1) / num_buckets))
    buckets = {}
    for i, l in enumerate(lens):
        buckets.setdefault((l - lo) // width, []).append(i)
    rng = np.random.default_rng(seed + epoch) if shuffle else None
    batches = []
    for k in sorted(buckets):
        idxs = buckets[k]
        if shuffle:
            idxs = [idxs[j] for j in rng.permutation(len(idxs))]
        batches += [idxs[s:s + batch_size] for s in range(0, len(idxs), batch_size)]
    if shuffle:
        batches = [batches[j] for j in rng.permutation(len(batches))]
    if world > 1:
        n = -(-len(batches) // world) * world
        batches = [batches[j % len(batches)] for j in range(n)][rank::world]
    if rows is not None:
        caps, clens = dataset.get_captions(ids=True), dataset.get_clip_lens()
        for ids in batches:
            tmax, lmax = max(clens[i] for i in ids), max(len(caps[i]) for i in ids)
            tgt = np.zeros((len(ids), lmax), np.int32)
            for j, i in enumerate(ids):
                tgt[j, :len(caps[i])] = caps[i]
            batch = (np.ascontiguousarray(rows[ids, :tmax], dtype=np.int32), tgt, np.array([clens[i] for i in ids], np.float32),
                     np.array([len(caps[i]) for i in ids], np.float32))
            yield batch + (np.array(ids, np.int64),) if dataset._inference else batch
        return
    tf = getattr(dataset, "_transform", None)
    for ids in batches:
        batch = pad_batchify([dataset[i] for i in ids])
        if getattr(tf, "device_batched", False) and batch[0].dtype == np.uint8:
            batch = (tf(batch[0]),) + batch[1:]      # frame source: one transform launch group per batch, (B, T, S, S, 3) uint8 on the GPU
        yield batch


def to_device(src):
    """a batch's source as ``bucketed_batches`` yields it - a host array, or frames the transform already left on the GPU"""
    return src.cuda() if isinstance(src, torch.Tensor) else torch.from_numpy(src).cuda()


def write_sentences(sentences, file_path):                             # utils/captioning.py:89-95
    with io.open(file_path, "w", encoding="utf-8") as of:
        for sent in sentences:
            of.write((u" ".join(sent) if isinstance(sent, (list, tuple)) else sent) + u"\n")


def alignment_record(inst_id, attention, sample_valid_length, src_valid_length):
    """One instance's record for ``evaluate(alignments=...)``: ``(instance id, weights (words, T_valid) float32)`` from the best beam's
    attention rows ``attention`` (L - 1, T).  Row ``j`` belongs to token ``j + 1`` of the sample; ``evaluate`` writes out tokens
    ``1 .. sample_valid_length - 2`` (between <bos> and <eos>), so rows ``0 .. sample_valid_length - 3`` stay, cut to the clip's valid steps."""
    words = max(int(sample_valid_length) - 2, 0)
    tv = max(min(int(round(float(src_valid_length))), attention.shape[1]), 0)
    return int(inst_id), np.ascontiguousarray(attention[:words, :tv], dtype=np.float32)


def save_alignments(file_path, records, frame_ids=None):
    """``evaluate(alignments=...)``'s records as one ``.npz`` of flat arrays (``np.load(..., allow_pickle=False)`` reads it):
    ``inst_ids`` (N,), ``words`` / ``steps`` (N,) = each record's shape, ``offsets`` (N + 1,) into ``weights`` (the records' rows,
    concatenated and flattened), ``word_offsets`` (N + 1,) into ``argmax`` (the source step with the largest weight, per word), and -
    with ``frame_ids`` = {instance id: the (video, frame number) of each source step, as ``CaptionSet.clip_frames`` / ``clip_table``
    name it} - ``frame_offsets`` (N + 1,) into ``frame_videos`` (strings) and ``frame_numbers`` (int64).
    Records are written in instance-id order."""
    records = sorted(records, key=lambda r: r[0])
    ids = np.array([r[0] for r in records], np.int64)
    words = np.array([r[1].shape[0] for r in records], np.int64)
    steps = np.array([r[1].shape[1] for r in records], np.int64)
    offsets = np.concatenate([[0], np.cumsum(words * steps)]).astype(np.int64)
    word_offsets = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
    weights = np.concatenate([r[1].reshape(-1) for r in records]).astype(np.float32) if records else np.zeros(0, np.float32)
    argmax = np.concatenate([r[1].argmax(axis=1) if r[1].size else np.zeros(r[1].shape[0], np.int64)
                             for r in records]).astype(np.int32) if records else np.zeros(0, np.int32)
    out = dict(inst_ids=ids, words=words, steps=steps, offsets=offsets, weights=weights, word_offsets=word_offsets, argmax=argmax)
    if frame_ids is not None:
        clips = [list(frame_ids[int(i)]) for i in ids]
        out["frame_offsets"] = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
        flat = [vf for c in clips for vf in c]
        out["frame_videos"] = np.array([str(v) for v, _ in flat], dtype=np.str_) if flat else np.zeros(0, "<U1")
        out["frame_numbers"] = np.array([int(f) for _, f in flat], np.int64)
    np.savez(file_path, **out)


def load_alignments(file_path):
    """-> [(instance id, weights (words, steps), argmax (words,), [(video, frame number)] or None)] from ``save_alignments``' file."""
    with np.load(file_path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    out = []
    for n, i in enumerate(d["inst_ids"]):
        w = d["weights"][d["offsets"][n]:d["offsets"][n + 1]].reshape(int(d["words"][n]), int(d["steps"][n]))
        am = d["argmax"][d["word_offsets"][n]:d["word_offsets"][n + 1]]
        fo = d["frame_offsets"][n:n + 2] if "frame_offsets" in d else None
        fr = None if fo is None else list(zip(d["frame_videos"][fo[0]:fo[1]].tolist(), d["frame_numbers"][fo[0]:fo[1]].tolist()))
        out.append((int(i), w, am, fr))
    return out


def clip_frame_ids(dataset):
    """{instance id: [(video, frame number)] per source step} of a ``CaptionSet`` (``clip_frames``; ``clip_table``'s
    ``frames[idx[i, t]]`` is the same pair): what ``save_alignments`` stores next to the weights."""
    return {i: dataset.clip_frames(i) for i in range(len(dataset))}


def evaluate(data_loader, model, translator, data_train, table=None, alignments=None):
    """reference train_gnmt.py:264-302: teacher-forced MaskedSoftmaxCELoss + beam search; returns
    (avg_loss, translations ordered by instance id).  Everything numeric runs on the GPU.
    ``table``: the split's device-resident feature table; a loader that yields table rows (``bucketed_batches(rows=...)``: an int32
    (B, T) source) is then encoded by ``encode_rows`` / ``translate_rows``, with the same results.
    ``alignments``: a list; one ``alignment_record`` per instance is appended to it - the best beam's attention weights over the clip's
    valid steps, one row per word written out.  The return value does not change."""
    from .engine import masked_softmax_ce
    translation_out, all_inst_ids = [], []
    avg_loss_denom, avg_loss = 0, 0.0
    for src_seq, tgt_seq, src_valid_length, tgt_valid_length, inst_ids in data_loader:
        by_rows = isinstance(src_seq, np.ndarray) and src_seq.ndim == 2 and src_seq.dtype.kind == "i"
        if by_rows and table is None:
            raise ValueError("evaluate: the loader yields table rows but no feature table was given")
        src = src_seq if by_rows else model.embed_source(to_device(src_seq))    # frame mode: the clip's frames through the CNN
        tgt = torch.from_numpy(tgt_seq).cuda()
        svl = torch.from_numpy(src_valid_length).cuda()
        tvl = torch.from_numpy(tgt_valid_length).cuda()
        b, t = src.shape[0], src.shape[1]
        cap = model._captioner(translator._beam_size, translator._max_length, b, t)
        if by_rows:
            cap.encode_rows(table, src, src_valid_length)
        else:
            cap.encode(src, svl)
        out = cap.decode_seq(tgt[:, :-1])                              # model(src, tgt[:, :-1], ...)   :280
        loss = masked_softmax_ce(out, tgt[:, 1:], tvl - 1).mean().item()   # :281
        all_inst_ids.extend(inst_ids.astype(np.int32).tolist())
        avg_loss += loss * (tgt_seq.shape[1] - 1)
        avg_loss_denom += (tgt_seq.shape[1] - 1)
        if alignments is None:
            samples, _, sample_valid_length = (translator.translate_rows(table, src, src_valid_length) if by_rows
                                               else translator.translate(src, svl))   # :287-288
        else:
            samples, _, sample_valid_length, att = (translator.translate_rows(table, src, src_valid_length, return_attention=True)
                                                    if by_rows else translator.translate(src, svl, return_attention=True))
        max_score_sample = samples[:, 0, :].cpu().numpy()
        svl0 = sample_valid_length[:, 0].cpu().numpy()
        if alignments is not None:
            att0 = att[:, 0].cpu().numpy()
            for i in range(att0.shape[0]):
                alignments.append(alignment_record(inst_ids[i], att0[i], svl0[i], src_valid_length[i]))
        for i in range(max_score_sample.shape[0]):                     # :291-294
            translation_out.append([data_train.vocab.idx_to_token[ele]
                                    for ele in max_score_sample[i][1:(svl0[i] - 1)]])
    avg_loss = avg_loss / avg_loss_denom
    real_translation_out = [None for _ in range(len(all_inst_ids))]
    for ind, sentence in zip(all_inst_ids, translation_out):           # :298-300
        real_translation_out[ind] = sentence
    return avg_loss, real_translation_out
