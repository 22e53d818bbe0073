"""Model specifications — mirror of reference models/vision/definitions.py.

Same class names, constructor arguments and attributes (``backbone``, ``classes``,
``td``, ``rnn``) as the reference; ``model(x)`` runs on the MI355X through
libtennis_hip.so.  Inputs may be numpy or torch tensors; outputs are torch CUDA
tensors (fp32), the counterpart of MXNet NDArrays on ``mx.gpu``.
"""
import numpy as np
import torch

from ...block import Block
from ...engine import WindowHead, temporal_pool, temporal_pool_rows, temporal_pool_windows
from ...nn import GRU, LSTM, Dense, _to_device
from ...utils.layers import TimeDistributed


WINDOW_MAX_ROWS = 1 << 18      # rows of the feature matrix one WindowHead projects at a time (its gi buffer: rows x 2*G*H fp32)


def _host_index(a):
    """an index array (numpy, list, or torch on any device) as int64 numpy"""
    return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a).astype(np.int64)


def window_chunks(centre, lo, hi, rows, max_rows):
    """Cuts a feature matrix of ``rows`` rows into pieces of at most ``max_rows`` at video boundaries: a sample never leaves
    ``[lo, hi]``, so whole videos are independent.  -> [(first row, end row, sample ids)]; one piece when the matrix fits."""
    centre, lo, hi = (_host_index(a) for a in (centre, lo, hi))
    if rows <= max_rows:
        return [(0, rows, np.arange(len(centre)))]
    if np.any(lo < 0) or np.any(hi >= rows) or np.any(lo > hi):
        raise ValueError("a matrix larger than the row budget is cut at video boundaries: every [lo, hi] must lie inside it")
    segs = np.unique(np.stack([lo, hi], 1), axis=0)            # sorted by lo
    if np.any(segs[1:, 0] <= segs[:-1, 1]):
        raise ValueError("a matrix larger than the row budget is cut at video boundaries: the [lo, hi] ranges overlap")
    pieces, first, end = [], int(segs[0, 0]), int(segs[0, 0])
    for a, b in segs:
        if b + 1 - a > max_rows:
            raise ValueError(f"a video of {b + 1 - a} rows does not fit the row budget of {max_rows}")
        if b + 1 - first > max_rows:
            pieces.append((first, end))
            first = int(a)
        end = int(b) + 1
    pieces.append((first, end))
    return [(a, b, np.nonzero((lo >= a) & (hi < b))[0]) for a, b in pieces]


def table_chunks(idx, row_videos, max_rows):
    """``window_chunks`` for a row table (``TennisSet.window_table``): cuts a table of ``len(row_videos)`` rows into pieces of at most
    ``max_rows`` whole videos.  ``idx`` (samples, window): the rows every sample reads; ``row_videos``: the video of every row of the
    table - a sample's rows never leave its video, and the table is sorted by (video, frame), so a video is one run of rows.
    -> [(first row, end row, sample ids, idx[sample ids] - first row)]; one piece when the table fits."""
    idx = _host_index(idx)
    rows = len(row_videos)
    if idx.ndim != 2:
        raise ValueError(f"the row table must be (samples, window), got {idx.shape}")
    if rows <= max_rows:
        return [(0, rows, np.arange(len(idx)), idx)]
    if len(idx) and (idx.min() < 0 or idx.max() >= rows):
        raise ValueError("a table larger than the row budget is cut at video boundaries: every index must lie inside it")
    starts = [0] + [r for r in range(1, rows) if row_videos[r] != row_videos[r - 1]]
    if len({row_videos[a] for a in starts}) != len(starts):
        raise ValueError("a table larger than the row budget is cut at video boundaries: the rows of a video are not contiguous")
    ends = starts[1:] + [rows]
    lo, hi = idx.min(1), idx.max(1)
    seg = np.searchsorted(np.asarray(starts), lo, side="right") - 1            # the video run each sample's first row lies in
    if np.any(hi >= np.asarray(ends)[seg]):
        raise ValueError("a table larger than the row budget is cut at video boundaries: a sample reads rows of two videos")
    pieces, first = [], 0
    for a, b in zip(starts, ends):
        if b - a > max_rows:
            raise ValueError(f"a video of {b - a} rows does not fit the row budget of {max_rows}")
        if b - first > max_rows:
            pieces.append((first, a))
            first = a
    pieces.append((first, rows))
    out = []
    for a, b in pieces:
        ids = np.nonzero((lo >= a) & (hi < b))[0]
        out.append((a, b, ids, idx[ids] - a))
    return out


def _need_classes(model, what):
    if not model.classes:
        raise ValueError(f"{what}(..., return_tam=True) needs a model with classes (num_classes > 0): the maps are those of its Dense")


def _scatter(out, ids, y, n):
    """out[ids] = y for the pieces of a cut matrix; ``out`` (n, ...) is created from the first piece"""
    if out is None:
        out = torch.empty((n,) + tuple(y.shape[1:]), dtype=y.dtype, device=y.device)
    out[torch.from_numpy(ids).to(y.device)] = y
    return out


class FrameModel(Block):
    """Reference definitions.py:10-33: backbone CNN + one Dense to the classes."""

    def __init__(self, backbone, num_classes=-1, swap=False, **kwargs):
        super().__init__(**kwargs)
        if swap:
            raise NotImplementedError("swap=True is the R(2+1)D path (reference evaluate.py:132), out of scope")
        self.swap = swap
        self.backbone = backbone
        self.classes = None
        if num_classes > 0:
            self.classes = Dense(num_classes, flatten=True, prefix=self.prefix + "dense0_")

    def forward(self, x, return_cam=False):
        """``return_cam=True``: ``(logits, cam)`` with ``cam`` ``(B, classes, h, w)`` the class activation maps of the same
        forward (7 x 7 cells per pool window: 7 x 7 at 224^2, 14 x 14 at 512^2) - ``classes.bias[c] + cam[b, c].sum()`` is
        ``logits[b, c]``, exactly in real arithmetic (the network ends in BN, ReLU, average pool, Dense: CAM, no backward pass).
        The logits are those of ``forward(x)``, bit for bit.  Needs a model with ``classes``."""
        if return_cam:
            if not self.classes:
                raise ValueError("return_cam=True needs a FrameModel with classes (num_classes > 0): the maps are those of its Dense")
            feat, cam = self.backbone(x, class_maps=self.classes.engine_for)
            return self.classes(feat), cam
        x = self.backbone(x)            # definitions.py:30
        if self.classes:
            x = self.classes(x)         # definitions.py:31-32
        return x


class TemporalPooling(Block):
    """Reference definitions.py:36-72."""

    def __init__(self, model, num_classes=-1, pool="max", feats=False, **kwargs):
        super().__init__(**kwargs)
        self.pool = pool
        self.feats = feats
        self.classes = None
        if model is not None:
            if num_classes == 0:                       # definitions.py:53-55
                self.td = TimeDistributed(model.backbone)
                self.classes = model.classes
            else:                                      # definitions.py:56-59
                self.td = TimeDistributed(model)
                if num_classes > 0:
                    self.classes = Dense(num_classes, flatten=True, prefix=self.prefix + "dense0_")
        else:                                          # definitions.py:60-61
            self.classes = Dense(num_classes, flatten=True, prefix=self.prefix + "dense0_")

    def _tam_check(self, what):
        """``return_tam`` is for the max pool of a model with classes"""
        if self.pool == "mean":
            raise ValueError(f"{what}(..., return_tam=True) is for pool='max': a mean reads every step alike - its decomposition is the "
                             "Dense applied to each step's features and divided by the window, which needs no step bookkeeping and "
                             "which a caller can already compute; it is out of scope here")
        _need_classes(self, what)

    def _maps(self, y, steps, window):
        """the Dense and its maps for pooled features ``y`` and their steps -> (logits, tam)"""
        y = y.reshape(y.shape[0], -1)
        return self.classes(y), self.classes.engine_for(y.shape[1]).step_maps(y, steps, window)

    def forward(self, x, return_tam=False):
        """``return_tam=True``: ``(logits, tam)`` with ``tam`` ``(N, classes, window)`` the temporal activation maps of the same
        forward: the model ends in ``max over the window -> Dense``, so ``classes.bias[c] + tam[n, c].sum()`` is ``logits[n, c]``
        exactly in real arithmetic, ``tam[n, c, t]`` being the part of the Dense's sum read from window step ``t`` (no backward
        pass).  The logits are those of ``forward(x)``, bit for bit.  ``pool="max"`` and a model with ``classes`` only."""
        if return_tam:
            self._tam_check("forward")
        if not self.feats:
            x = self.td(x)                             # definitions.py:64-65
        if return_tam:
            x = _to_device(x)
            return self._maps(*temporal_pool(x, "max", return_steps=True), x.shape[1])
        x = temporal_pool(_to_device(x), "mean" if self.pool == "mean" else "max")   # :66-69
        if self.classes:
            x = self.classes(x)
        return x

    def forward_windows(self, features, centre, lo, hi, window, stride=1, max_rows=WINDOW_MAX_ROWS, return_tam=False):
        """``forward`` of every window of a (rows, F) feature matrix without materialising the (samples, window, F) batch: sample
        ``b`` pools the rows ``clamp(centre[b] + (t - window // 2) * stride, lo[b], hi[b])``, t = 0 .. window-1
        (``TennisSet.window_rows``) -> logits (samples, classes).  Feature mode only.  ``return_tam`` as in ``forward``."""
        if return_tam:
            self._tam_check("forward_windows")
        if not self.feats:
            raise NotImplementedError("forward_windows: feature mode only (TemporalPooling(..., feats=True))")
        x = _to_device(features).float()
        if x.dim() != 2:
            raise ValueError(f"forward_windows expects a (rows, F) feature matrix, got {tuple(x.shape)}")
        kind = "mean" if self.pool == "mean" else "max"
        out, tam, n = None, None, len(_host_index(centre))
        for a, b, ids in window_chunks(centre, lo, hi, x.shape[0], max_rows):
            c, l, h = (_host_index(v)[ids] - a for v in (centre, lo, hi))
            if return_tam:
                y, t = self._maps(*temporal_pool_windows(x[a:b], c, l, h, window, stride, "max", return_steps=True), window)
                out, tam = _scatter(out, ids, y, n), _scatter(tam, ids, t, n)
                continue
            y = temporal_pool_windows(x[a:b], c, l, h, window, stride, kind)
            if self.classes:
                y = self.classes(y)
            if out is None:
                out = torch.empty((len(_host_index(centre)), y.shape[1]), dtype=torch.float32, device=y.device)
            out[torch.from_numpy(ids).to(y.device)] = y
        return (out, tam) if return_tam else out

    def forward_table(self, features, idx, max_rows=WINDOW_MAX_ROWS, row_videos=None, return_tam=False):
        """``forward`` of every window named by a row table (``TennisSet.window_table``): sample ``b`` pools the rows ``idx[b, t]`` of
        ``features`` (rows, F), t ascending -> logits (samples, classes).  Feature mode: ``features`` are the stored features.
        Frames mode: the rows ``self.td.model`` produced for the table's frames, each frame encoded once
        (``evaluate.encode_table``).  Any sample layout; ``row_videos`` (the video of every row) is needed only to cut a table of
        more than ``max_rows`` rows.  ``return_tam`` as in ``forward``."""
        if return_tam:
            self._tam_check("forward_table")
        x = _to_device(features).float()
        if x.dim() != 2:
            raise ValueError(f"forward_table expects a (rows, F) feature matrix, got {tuple(x.shape)}")
        kind = "mean" if self.pool == "mean" else "max"
        if x.shape[0] > max_rows and row_videos is None:
            raise ValueError(f"forward_table: a table of {x.shape[0]} rows over the budget of {max_rows} needs row_videos to be cut")
        out, tam, n = None, None, len(_host_index(idx))
        for a, b, ids, local in table_chunks(idx, row_videos if row_videos is not None else [0] * x.shape[0], max_rows):
            if not len(ids):
                continue
            if return_tam:
                y, t = self._maps(*temporal_pool_rows(x[a:b], local, "max", return_steps=True), local.shape[1])
                out, tam = _scatter(out, ids, y, n), _scatter(tam, ids, t, n)
                continue
            y = temporal_pool_rows(x[a:b], local, kind)
            if self.classes:
                y = self.classes(y)
            if out is None:
                out = torch.empty((n, y.shape[1]), dtype=torch.float32, device=y.device)
            out[torch.from_numpy(ids).to(y.device)] = y
        return (out, tam) if return_tam else out


class CNNRNN(Block):
    """Reference definitions.py:75-110: [TimeDistributed CNN ->] bi-GRU/LSTM -> max over T -> Dense."""

    def __init__(self, model, num_classes=-1, hidden_size=128, type="gru", **kwargs):
        super().__init__(**kwargs)
        self.feats = model is None
        if model is not None:
            self.td = TimeDistributed(model.backbone)                  # definitions.py:91-92
        if type == "lstm":                                             # definitions.py:93-96
            self.rnn = LSTM(hidden_size, layout="NTC", bidirectional=True, prefix=self.prefix + "lstm0_")
        else:
            self.rnn = GRU(hidden_size, layout="NTC", bidirectional=True, prefix=self.prefix + "gru0_")
        self.classes = None
        if num_classes == 0:                                           # definitions.py:98-101
            self.classes = model.classes
        elif num_classes > 0:
            self.classes = Dense(num_classes, flatten=True, prefix=self.prefix + "dense0_")

    def forward(self, x, return_tam=False):
        """``return_tam=True``: ``(logits, tam)`` with ``tam`` ``(N, classes, window)`` the temporal activation maps of the same
        forward: the model ends in ``max over the window -> Dense``, so ``classes.bias[c] + tam[n, c].sum()`` is ``logits[n, c]``
        exactly in real arithmetic, ``tam[n, c, t]`` being the part of the Dense's sum read from the recurrent state of window step
        ``t`` (no backward pass).  A state at step ``t`` has seen the steps before it (after it, in the reverse direction): the maps
        say which step's state a logit was read from, not which single frame caused it.  The logits are those of ``forward(x)``, bit
        for bit.  Needs a model with ``classes``."""
        if return_tam:
            _need_classes(self, "forward")
        if not self.feats:
            x = self.td(x)                                             # definitions.py:104-105
        x = self.rnn(x)                                                # :106
        if return_tam:
            pooled, steps = temporal_pool(x, "max", return_steps=True)
            return self.classes(pooled), self.classes.engine_for(pooled.shape[1]).step_maps(pooled, steps, x.shape[1])
        x = temporal_pool(x, "max")                                    # :107
        if self.classes:
            x = self.classes(x)                                        # :108-109
        return x

    def forward_windows(self, features, centre, lo, hi, window, stride=1, max_rows=WINDOW_MAX_ROWS, return_tam=False):
        """``forward`` of every window of a (rows, F) feature matrix with ONE i2h projection per row (``engine.WindowHead``): sample
        ``b`` runs over the rows ``clamp(centre[b] + (t - window // 2) * stride, lo[b], hi[b])``, t = 0 .. window-1
        (``TennisSet.window_rows``) -> logits (samples, classes).  Feature mode only.  A matrix of more than ``max_rows`` rows is cut
        at video boundaries.  ``return_tam`` as in ``forward``: the maps come out of the windowed kernel's own pass."""
        if return_tam:
            _need_classes(self, "forward_windows")
        if not self.feats:
            raise NotImplementedError("forward_windows: feature mode only (CNNRNN(model=None, ...))")
        if not self.classes:
            raise NotImplementedError("forward_windows returns logits: the model needs its Dense (num_classes > 0)")
        x = _to_device(features).float()
        if x.dim() != 2:
            raise ValueError(f"forward_windows expects a (rows, F) feature matrix, got {tuple(x.shape)}")
        n = len(_host_index(centre))
        self.rnn._materialize(x.shape[1])
        self.classes._materialize(2 * self.rnn._hidden)
        pieces = window_chunks(centre, lo, hi, x.shape[0], max_rows)
        eng = self._window_head(x.shape[1], max(b - a for a, b, _ in pieces), max(len(ids) for _, _, ids in pieces))
        if len(pieces) == 1:
            return eng.project(x).forward(centre, lo, hi, window, stride, return_tam=return_tam)
        out = torch.empty((n, self.classes._units), dtype=torch.float32, device=x.device)
        tam = torch.empty((n, self.classes._units, int(window)), dtype=torch.float32, device=x.device) if return_tam else None
        for a, b, ids in pieces:
            c, l, h = (_host_index(v)[ids] - a for v in (centre, lo, hi))
            at = torch.from_numpy(ids).to(x.device)
            if return_tam:
                out[at], tam[at] = eng.project(x[a:b]).forward(c, l, h, window, stride, return_tam=True)
            else:
                out[at] = eng.project(x[a:b]).forward(c, l, h, window, stride)
        return (out, tam) if return_tam else out


    def _window_head(self, width, need_rows, need_samples):
        """the ``WindowHead`` of this model's parameters, rebuilt when it is too small for the piece at hand"""
        eng = self._engine
        if eng is None or eng.max_rows < need_rows or eng.max_samples < need_samples or eng.input_size != width:
            self._engine = eng = None      # release the old workspace first
            p = {k: v.data for blk in (self.rnn, self.classes) for k, v in blk._own_params.items()}
            self._engine = eng = WindowHead(self.rnn._mode, width, self.rnn._hidden, self.classes._units, p, self.rnn.prefix,
                                            self.classes.prefix, max_rows=need_rows, max_samples=need_samples)
        return eng

    def forward_table(self, features, idx, max_rows=WINDOW_MAX_ROWS, row_videos=None, return_tam=False):
        """``forward`` of every window named by a row table (``TennisSet.window_table``) with ONE i2h projection per row: sample ``b``
        runs over the rows ``idx[b, t]`` of ``features`` (rows, F), t = 0 .. window-1 -> logits (samples, classes).  Feature mode:
        ``features`` are the stored features.  Frames mode: the rows ``self.td.model`` (the model's own backbone) produced for the
        table's frames, each frame encoded once (``evaluate.encode_table``); their width must be the recurrent layer's input size.
        Any sample layout.  A table of more than ``max_rows`` rows is cut into pieces of whole videos, which needs ``row_videos``
        (the video of every row of the table).  ``return_tam`` as in ``forward``."""
        if return_tam:
            _need_classes(self, "forward_table")
        if not self.classes:
            raise NotImplementedError("forward_table returns logits: the model needs its Dense (num_classes > 0)")
        x = _to_device(features).float()
        if x.dim() != 2:
            raise ValueError(f"forward_table expects a (rows, F) feature matrix, got {tuple(x.shape)}")
        self.rnn._materialize(x.shape[1])
        if self.rnn._input_size != x.shape[1]:
            raise ValueError(f"forward_table: feature rows of width {x.shape[1]}, the recurrent layer takes {self.rnn._input_size}")
        self.classes._materialize(2 * self.rnn._hidden)
        if x.shape[0] > max_rows and row_videos is None:
            raise ValueError(f"forward_table: a table of {x.shape[0]} rows over the budget of {max_rows} needs row_videos to be cut")
        pieces = table_chunks(idx, row_videos if row_videos is not None else [0] * x.shape[0], max_rows)
        eng = self._window_head(x.shape[1], max(b - a for a, b, _, _ in pieces), max(max(len(ids) for _, _, ids, _ in pieces), 1))
        if len(pieces) == 1:
            return eng.project(x).forward_rows(pieces[0][3], return_tam=return_tam)
        n, window = _host_index(idx).shape
        out = torch.empty((n, self.classes._units), dtype=torch.float32, device=x.device)
        tam = torch.empty((n, self.classes._units, window), dtype=torch.float32, device=x.device) if return_tam else None
        for a, b, ids, local in pieces:
            if not len(ids):
                continue
            at = torch.from_numpy(ids).to(x.device)
            if return_tam:
                out[at], tam[at] = eng.project(x[a:b]).forward_rows(local, return_tam=True)
            else:
                out[at] = eng.project(x[a:b]).forward_rows(local)
        return (out, tam) if return_tam else out


class TwoStreamModel(Block):
    """Reference definitions.py:127-153 — optical-flow two-stream input is out of the
    hot path (needs 217 GB of flow JPEGs + FlowNet weights)."""

    def __init__(self, *a, **k):
        raise NotImplementedError("TwoStreamModel (flow input) is outside the accelerated hot path")
