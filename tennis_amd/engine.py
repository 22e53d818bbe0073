"""Device-side building blocks: thin Python handles over the C ABI.

Each class owns one opaque library handle (weights + workspace live in HBM
inside it) and launches on the Context's HIP stream.  Tensors crossing this
boundary are torch CUDA tensors used purely as device buffers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr


def _on_ctx_device(ctx, x: torch.Tensor, what: str):
    """A handle's weights and workspace live on its context's GPU: inputs must be there too (one process per GPU)."""
    if not x.is_cuda:
        raise ValueError(f"{what}: input must already be on the GPU")
    if x.device.index != ctx.device:
        raise ValueError(f"{what}: input is on cuda:{x.device.index} but this handle was built on cuda:{ctx.device}")


def _clip_table(ctx, table: torch.Tensor, input_size: int, what: str) -> torch.Tensor:
    """The (rows, F) fp32 feature table the captioner's ``*_rows`` calls gather their clips from: on the handle's GPU already (uploaded
    once), rows of unit element stride - a column slice of a wider table passes, its row stride travels as ``ld``."""
    if not isinstance(table, torch.Tensor):
        raise ValueError(f"{what}: the table must be a torch tensor on the GPU, got {type(table).__name__}")
    _on_ctx_device(ctx, table, what)
    if table.dim() != 2 or table.shape[1] != input_size or table.shape[0] < 1 or table.dtype != torch.float32:
        raise ValueError(f"{what}: need a (rows, {input_size}) float32 table, got {tuple(table.shape)} {table.dtype}")
    if table.stride(1) != 1 or table.stride(0) < input_size:
        table = table.contiguous()
    return table


def _clip_rows(ctx, table: torch.Tensor, idx, valid_length, what: str) -> torch.Tensor:
    """(B, T) clip rows -> int32 on the handle's GPU.  A host-side ``idx`` (numpy array, CPU tensor, nested list) is checked here,
    before any launch: -1 <= idx < rows, and no -1 (a pad step) before a clip's valid length.  A device tensor is passed through: the
    kernels read zeros for a negative index and clamp one past the table."""
    if isinstance(idx, torch.Tensor) and idx.is_cuda:
        _on_ctx_device(ctx, idx, what)
    else:
        host = idx.numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
        if host.dtype.kind not in "iu":
            raise ValueError(f"{what}: idx must hold integers, got {host.dtype}")
        if host.ndim != 2:
            raise ValueError(f"{what}: idx must be (batch, steps), got {host.shape}")
        if host.size and (int(host.min()) < -1 or int(host.max()) >= table.shape[0]):
            raise ValueError(f"{what}: idx must lie in [-1, {table.shape[0] - 1}], got [{int(host.min())}, {int(host.max())}]")
        vl = valid_length.detach().cpu().numpy() if isinstance(valid_length, torch.Tensor) else np.asarray(valid_length)
        vl = np.rint(vl).astype(np.int64).reshape(-1)
        if vl.shape[0] != host.shape[0] or (vl.size and (int(vl.min()) < 0 or int(vl.max()) > host.shape[1])):
            raise ValueError(f"{what}: valid lengths must be one per clip within [0, {host.shape[1]}]")
        inside = np.arange(host.shape[1])[None, :] < vl[:, None]
        if bool(((host < 0) & inside).any()):
            b = int(np.argmax(((host < 0) & inside).any(1)))
            raise ValueError(f"{what}: clip {b} has a pad step (-1) before its valid length {int(vl[b])}")
        idx = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(table.device)
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"{what}: idx must be (batch, steps), got {tuple(idx.shape)}")
    return idx.to(torch.int32).contiguous()


def _layout_of(x: torch.Tensor, size_hw):
    """Pick the tn_layout of a frame batch from dtype/shape (reference frames are
    NCHW float32 after ToTensor+Normalize, evaluate.py:96-97)."""
    h, w = size_hw
    if x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and tuple(x.shape[2:]) == (h, w):
        return _lib.LAYOUT_NCHW_F32
    if x.dtype == torch.float16 and x.dim() == 4 and x.shape[3] == 3 and tuple(x.shape[1:3]) == (h, w):
        return _lib.LAYOUT_NHWC_F16
    if x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3 and tuple(x.shape[1:3]) == (h, w):
        return _lib.LAYOUT_NHWC_U8
    raise ValueError(f"unsupported frame batch: shape {tuple(x.shape)} dtype {x.dtype} for a {h}x{w} encoder "
                     "(expected NCHW float32, NHWC float16 or NHWC uint8)")


def _device_view(ctx, addr, shape):
    """torch view of an fp32 device buffer owned by the library (for all-reduce / inspection)"""
    class _Arr:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (addr, False), "version": 3}
    return torch.as_tensor(_Arr(), device=f"cuda:{ctx.device}")


class _Handle:
    """Owns one library handle on a context; ``_ABI`` is the prefix of its C entry points (``tn_dense`` -> ``tn_dense_destroy``)."""
    _ABI = ""
    handle = None

    def __init__(self, ctx: _lib.Context | None = None):
        self.ctx = ctx or _lib.default_context()
        self.lib = self.ctx.lib

    def __del__(self):
        try:
            if self.handle:
                getattr(self.lib, self._ABI + "_destroy")(self.handle)
                self.handle = None
        except Exception:
            pass


class _FlatTrainer(_Handle):
    """A training handle whose parameters and gradients live in flat device buffers (``<_ABI>_buffers``) and are read back by
    name (``<_ABI>_read_param``).  ``_PARTS`` = 2: a backbone and the part on top of it, each with buffers of its own -
    ``params`` / ``grads`` are then tuples, and ``grads`` leaves a ``frozen`` backbone's out."""
    _PARTS = 1
    frozen = False

    def _select(self, params: dict, *prefixes):
        """Records ``names`` / ``shapes`` of the parameters under ``prefixes`` -> (tn_param array, keep-alive list)"""
        self.names = [k for k in params if k.startswith(prefixes)]
        self.shapes = {k: tuple(np.asarray(params[k]).shape) for k in self.names}
        return _lib.make_params({k: params[k] for k in self.names})

    def _adopt(self, h):
        """Owns the created handle ``h`` and asks for its flat buffers: (params address, grads address, numel) per part"""
        self.handle = h
        out = [c() for _ in range(self._PARTS) for c in (C.c_void_p, C.c_void_p, C.c_int64)]
        check(getattr(self.lib, self._ABI + "_buffers")(h, *[C.byref(o) for o in out]), self._ABI + "_buffers")
        self._parts = [tuple(o.value for o in out[3 * i:3 * i + 3]) for i in range(self._PARTS)]
        if self._PARTS == 1:
            self.numel = self._parts[0][2]

    def _views(self, which: int, trainable_only: bool = False):
        v = [_device_view(self.ctx, p[which], (p[2],)) for p in self._parts]
        if self._PARTS == 1:
            return v[0]
        return tuple(v[1:] if trainable_only and self.frozen else v)

    @property
    def grads(self):
        return self._views(1, True)

    @property
    def params(self):
        return self._views(0)

    def get(self, name: str, gradient: bool = False, shape=None) -> np.ndarray:
        shape = shape or self.shapes[name]
        out = np.empty(int(np.prod(shape)), np.float32)
        n = C.c_int64()
        check(getattr(self.lib, self._ABI + "_read_param")(self.handle, name.encode(), 1 if gradient else 0,
                                                           out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n)),
              self._ABI + "_read_param")
        return out[:n.value].reshape(shape if n.value == out.size else (n.value,)).copy()

    def state_dict(self) -> dict:
        """Every recorded parameter (for a backbone: its running statistics too), by name."""
        return {k: self.get(k) for k in self.names}

    def set_clip(self, max_norm: float):
        """Global-norm gradient clipping of ``step`` (``gluon.utils.clip_global_norm``): the update runs on ``scale * g`` with
        ``scale = min(1, max_norm / (norm + 1e-8))``, ``norm`` over every trainable gradient element (for the SGD trainers: of
        ``rescale_grad * g``; for the two-part trainers: over both parts).  ``grads`` stay unclipped.  0 switches it off, which is
        the state after construction; negative or non-finite values raise."""
        check(getattr(self.lib, self._ABI + "_set_clip")(self.handle, float(max_norm)), self._ABI + "_set_clip")

    def clip_stats(self) -> tuple:
        """(norm, scale) of the last clipped ``step`` and the steps with ``scale < 1`` since construction.  Synchronises the stream:
        for a log point, not for every step.  Raises while clipping is off or before a clipped step."""
        n, sc, k = C.c_float(), C.c_float(), C.c_int64()
        check(getattr(self.lib, self._ABI + "_clip_stats")(self.handle, C.byref(n), C.byref(sc), C.byref(k)), self._ABI + "_clip_stats")
        return n.value, sc.value, k.value


class DenseNet121Features(_Handle):
    """``get_model('DenseNet121').features`` on the GPU (reference evaluate.py:125)."""

    _ABI = "tn_densenet121"

    def __init__(self, params: dict, size: int | tuple = 224, max_batch: int = 256, prefix: str = "densenet0_",
                 ctx: _lib.Context | None = None, exact_weights: bool = False, fp32: bool = False, fp32x3: bool = False):
        """``exact_weights``: keep the fp32 convolution weights of the dense layers / transitions as hi + lo fp16
        pairs (TN_ENC_EXACT_WEIGHTS) instead of rounding them to fp16 once — for parameters that were NOT converted
        with ``weights.as_fp16_model`` (a trained fp32 checkpoint) and a 1e-3 agreement with their fp32 evaluation.
        ``fp32``: the fp32 mode (TN_ENC_FP32) - fp32 weights, fp32 activations, every product in fp32: the fp32 evaluation of
        any checkpoint within 1e-3, at the f32 matrix rate; ``read_tap`` and ``input_means`` are not available.
        ``fp32x3``: the fp32x3 mode (TN_ENC_FP32X3) - the fp32 mode's network and fp32 activations, every operand handed to the
        bf16 matrix pipe as three bf16 terms (six products per k-step): the same bar for any checkpoint, faster; not together
        with ``fp32``."""
        super().__init__(ctx)
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.max_batch = max_batch
        arr, keep = _lib.make_params({k: v for k, v in params.items() if k.startswith(prefix)})
        h = C.c_void_p()
        self.exact_weights, self.fp32, self.fp32x3 = bool(exact_weights), bool(fp32), bool(fp32x3)
        flags = (_lib.ENC_EXACT_WEIGHTS if exact_weights else 0) | (_lib.ENC_FP32 if fp32 else 0) | (_lib.ENC_FP32X3 if fp32x3 else 0)
        check(self.lib.tn_densenet121_create_ex(self.ctx.handle, arr, len(arr), prefix.encode(), self.size[0], self.size[1],
                                                max_batch, flags, C.byref(h)),
              "tn_densenet121_create")
        del keep
        self.handle = h
        self.feature_dim = self.lib.tn_densenet121_feature_dim(h)
        self.workspace_bytes = self.lib.tn_densenet121_workspace_bytes(h)

    def __call__(self, x: torch.Tensor, out: torch.Tensor | None = None, class_maps: "Dense | None" = None):
        """Features ``(B, F)``.  ``class_maps=<engine.Dense>`` (``F`` inputs, at most 64 units, same context): returns
        ``(features, maps)`` with ``maps`` ``(B, units, *class_map_dims)`` the class activation maps of that Dense
        (``tn_densenet121_forward_class_maps``): ``bias[c] + maps[b, c].sum()`` is logit ``c`` of frame ``b``.  The features are
        bit-identical to a call without maps; a pipelined call orders the maps with ``join`` as it orders the features."""
        _on_ctx_device(self.ctx, x, "DenseNet121Features")
        x = x.contiguous()
        layout = _layout_of(x, self.size)
        b = x.shape[0]
        if out is None:
            out = torch.empty((b, self.feature_dim), dtype=torch.float32, device=x.device)
        if class_maps is None:
            check(self.lib.tn_densenet121_forward(self.handle, ptr(x), layout, b, ptr(out)), "tn_densenet121_forward")
            return out
        if not isinstance(class_maps, Dense):
            raise TypeError(f"class_maps must be an engine.Dense, got {type(class_maps).__name__}")
        maps = torch.empty((b, class_maps.units) + self.class_map_dims, dtype=torch.float32, device=x.device)
        check(self.lib.tn_densenet121_forward_class_maps(self.handle, ptr(x), layout, b, ptr(out), class_maps.handle, ptr(maps)),
              "tn_densenet121_forward_class_maps")
        return out, maps

    @property
    def class_map_dims(self) -> tuple:
        """``(h, w)`` of a class activation map: 7 cells per pool window each way (7 x 7 at 224^2, 14 x 14 at 512^2)."""
        h, w = C.c_int(), C.c_int()
        check(self.lib.tn_densenet121_class_map_dims(self.handle, C.byref(h), C.byref(w)), "tn_densenet121_class_map_dims")
        return h.value, w.value

    def profile_class_maps(self, x: torch.Tensor, class_maps: "Dense"):
        """``profile`` of a forward with maps: the family ``class_maps`` beside ``head_bnrelu_avgpool7`` -> (list of dicts, features, maps)."""
        x = x.contiguous()
        layout = _layout_of(x, self.size)
        b = x.shape[0]
        out = torch.empty((b, self.feature_dim), dtype=torch.float32, device=x.device)
        maps = torch.empty((b, class_maps.units) + self.class_map_dims, dtype=torch.float32, device=x.device)
        stats = (_lib.TnKernelStat * 24)()
        n = C.c_int(0)
        check(self.lib.tn_dbg_profile_class_maps(self.handle, ptr(x), layout, b, ptr(out), class_maps.handle, ptr(maps), stats, 24, C.byref(n)),
              "tn_dbg_profile_class_maps")
        return [dict(name=stats[i].name.decode(), launches=stats[i].launches, ms=stats[i].ms,
                     flops=stats[i].flops, bytes=stats[i].bytes) for i in range(n.value)], out, maps

    def set_pipelined(self, on: bool = True):
        """Consecutive calls overlap on the library's side streams; the caller orders the results with ``join`` (see
        ``tn_densenet121_set_pipelined`` in include/tennis_hip.h)."""
        check(self.lib.tn_densenet121_set_pipelined(self.handle, 1 if on else 0), "tn_densenet121_set_pipelined")

    def join(self, lag: int = 0):
        """The context's stream waits for the last call (``lag=0``) or the one before it (``lag=1``)."""
        check(self.lib.tn_densenet121_join(self.handle, lag), "tn_densenet121_join")

    def profile(self, x: torch.Tensor):
        """One forward with every launch bracketed by HIP events -> list of dicts."""
        x = x.contiguous()
        layout = _layout_of(x, self.size)
        b = x.shape[0]
        out = torch.empty((b, self.feature_dim), dtype=torch.float32, device=x.device)
        stats = (_lib.TnKernelStat * 16)()
        n = C.c_int(0)
        check(self.lib.tn_densenet121_profile(self.handle, ptr(x), layout, b, ptr(out), stats, 16, C.byref(n)),
              "tn_densenet121_profile")
        return [dict(name=stats[i].name.decode(), launches=stats[i].launches, ms=stats[i].ms,
                     flops=stats[i].flops, bytes=stats[i].bytes) for i in range(n.value)], out

    def input_means(self, x: torch.Tensor, prefix: str = "densenet0_") -> dict:
        """Calibration statistics (``tn_densenet121_input_means``): ``{conv weight name: mean of every input channel of that
        convolution}`` over the frames ``x``, for the 119 convolutions behind the stem - what
        ``weights.as_fp16_model(params, input_means=...)`` needs."""
        from . import weights as W
        x = x.contiguous()
        layout = _layout_of(x, self.size)
        convs, _, _ = W.densenet121_layout()
        convs = [c for c in convs if c["kind"] != "stem"]
        buf = np.empty(sum(c["cin"] for c in convs), dtype=np.float32)
        n = C.c_int64(0)
        check(self.lib.tn_densenet121_input_means(self.handle, ptr(x), layout, x.shape[0], buf.ctypes.data_as(C.c_void_p), buf.size,
                                                  C.byref(n)), "tn_densenet121_input_means")
        assert n.value == buf.size
        out, o = {}, 0
        for c in convs:
            out[prefix + c["name"] + "_weight"] = buf[o:o + c["cin"]].copy()
            o += c["cin"]
        return out

    def read_tap(self, tap: str, batch: int) -> np.ndarray:
        buf = np.empty(self._tap_numel(batch), dtype=np.float32)
        n = C.c_size_t(0)
        check(self.lib.tn_densenet121_read_tap(self.handle, tap.encode(), batch,
                                               buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)),
              "tn_densenet121_read_tap")
        return buf[:n.value]

    def _tap_numel(self, batch):
        hs = (self.size[0] - 1) // 2 + 1
        ws = (self.size[1] - 1) // 2 + 1
        return batch * hs * ws * 64  # stem / stage1 taps are the largest



class Dense(_Handle):
    """``nn.Dense(units, flatten=True)`` (reference definitions.py:25)."""

    _ABI = "tn_dense"

    def __init__(self, weight: np.ndarray, bias: np.ndarray | None, ctx: _lib.Context | None = None):
        super().__init__(ctx)
        w = np.ascontiguousarray(weight, dtype=np.float32)
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        self.units, self.in_units = w.shape
        h = C.c_void_p()
        check(self.lib.tn_dense_create(self.ctx.handle, w.ctypes.data_as(C.c_void_p),
                                       None if b is None else b.ctypes.data_as(C.c_void_p),
                                       self.units, self.in_units, C.byref(h)), "tn_dense_create")
        self.handle = h

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        _on_ctx_device(self.ctx, x, "Dense")
        x = x.reshape(x.shape[0], -1).contiguous().float()
        if x.shape[1] != self.in_units:
            raise ValueError(f"Dense expects {self.in_units} input units, got {x.shape[1]}")
        y = torch.empty((x.shape[0], self.units), dtype=torch.float32, device=x.device)
        check(self.lib.tn_dense_forward(self.handle, ptr(x), x.shape[0], ptr(y)), "tn_dense_forward")
        return y

    def step_maps(self, pooled: torch.Tensor, steps: torch.Tensor, window: int) -> torch.Tensor:
        """Temporal activation maps of a head that ends in ``max over T -> this Dense``: ``pooled`` (B, in_units) what the Dense saw,
        ``steps`` (B, in_units) the window position each unit's maximum was read from (``temporal_pool(..., return_steps=True)``)
        -> ``tam`` (B, units, window) with ``tam[b, c, t]`` the sum of ``weight[c, k] * pooled[b, k]`` over the ``k`` with
        ``steps[b, k] == t``: ``bias[c] + tam[b, c].sum()`` is the logit.  A step outside ``[0, window)`` contributes nothing."""
        _on_ctx_device(self.ctx, pooled, "Dense.step_maps")
        pooled = pooled.reshape(pooled.shape[0], -1).contiguous().float()
        steps = steps.reshape(steps.shape[0], -1).to(device=pooled.device, dtype=torch.int32).contiguous()
        if pooled.shape[1] != self.in_units or steps.shape != pooled.shape:
            raise ValueError(f"Dense.step_maps expects pooled and steps of shape (B, {self.in_units}), got {tuple(pooled.shape)} and "
                             f"{tuple(steps.shape)}")
        tam = torch.empty((pooled.shape[0], self.units, int(window)), dtype=torch.float32, device=pooled.device)
        check(self.lib.tn_dense_step_maps(self.handle, ptr(pooled), ptr(steps), pooled.shape[0], int(window), ptr(tam)),
              "tn_dense_step_maps")
        return tam


def event_decoder_geometry():
    """``tn_dbg_event_decoder_geometry``: (positions per workgroup of the score kernel, tile counts per step of the one scan
    workgroup); touches no device."""
    tile, scan = C.c_int(), C.c_int()
    check(_lib.load().tn_dbg_event_decoder_geometry(C.byref(tile), C.byref(scan)), "tn_dbg_event_decoder_geometry")
    return tile.value, scan.value


def event_decoder_switch_geometry():
    """``tn_dbg_event_decoder_switch_geometry``: positions of a video the switch-cost path kernels take per step; touches no device."""
    tile = C.c_int()
    check(_lib.load().tn_dbg_event_decoder_switch_geometry(C.byref(tile)), "tn_dbg_event_decoder_switch_geometry")
    return tile.value


def event_decoder_transition_geometry():
    """``tn_dbg_event_decoder_transition_geometry``: (positions of a video the transition-matrix path kernels take per step, bytes of a
    position's back-pointer row in a handle of up to 16 classes, the same above 16); touches no device."""
    tile, p16, p64 = C.c_int(), C.c_int(), C.c_int()
    check(_lib.load().tn_dbg_event_decoder_transition_geometry(C.byref(tile), C.byref(p16), C.byref(p64)),
          "tn_dbg_event_decoder_transition_geometry")
    return tile.value, p16.value, p64.value


class EventDecoder(_Handle):
    """Per-frame logits -> events on the device (``tn_event_decoder_*``, docs/kernels.md "Event decoding"): workspace for up to
    ``max_positions`` positions of up to ``classes`` classes; ``decode`` allocates its outputs only."""

    _ABI = "tn_event_decoder"

    def __init__(self, max_positions: int, classes: int, ctx: _lib.Context | None = None):
        super().__init__(ctx)
        self.max_positions, self.classes = int(max_positions), int(classes)
        h = C.c_void_p()
        check(self.lib.tn_event_decoder_create(self.ctx.handle, self.max_positions, self.classes, C.byref(h)), "tn_event_decoder_create")
        self.handle = h

    def workspace_bytes(self) -> int:
        """``tn_dbg_event_decoder_workspace_bytes``: device bytes the handle holds (the path workspace of ``switch_cost``, the back-pointer
        workspace of ``transitions`` and the workspace of ``posteriors`` are each allocated by the first call that gives one)."""
        n = C.c_size_t()
        check(self.lib.tn_dbg_event_decoder_workspace_bytes(self.handle, C.byref(n)), "tn_dbg_event_decoder_workspace_bytes")
        return n.value

    def decode(self, logits: torch.Tensor, rows, start, smooth: int = 1, return_frames: bool = False, switch_cost: float | None = None,
               transitions=None, posteriors: bool = False, return_posteriors: bool = False):
        """``logits`` (N, C) fp32 on the GPU; ``rows`` (M,) the logit row of every position of the time-ordered list (clamped into
        ``[0, N)``), ``start`` (M,) non-zero where a video begins, ``smooth`` the odd window width in [1, 63].  Returns a dict of
        tensors on the GPU, one entry per event in order of ``first``: ``first``, ``last`` (positions, inclusive), ``cls`` (int32),
        ``score`` the mean and ``peak`` the maximum of the smoothed score of ``cls`` over the event (float32); with
        ``return_frames`` also ``label`` (M,) int32 and ``conf`` (M,) float32 of every position.  Synchronises once, for the count.
        ``switch_cost`` (finite, >= 0, in logit units; not together with ``smooth`` > 1): the labels are the path that maximises the
        summed scores minus ``switch_cost`` per change of label inside a video (``tn_event_decoder_run_switch``), ``conf`` the
        unsmoothed probability of the label; None: the call is what it was.
        ``transitions`` (a numpy array or CPU tensor (C, C), ``[from, to]``, every entry <= 0 or -inf, the diagonal finite; not together
        with ``smooth`` > 1 or ``switch_cost``): the labels are the path that maximises the summed scores plus ``transitions[a, b]`` for
        every position labelled ``b`` that follows one labelled ``a`` inside a video (``tn_event_decoder_run_transitions``), ``conf`` as
        with ``switch_cost``; None: the call is what it was.
        ``posteriors`` (with ``transitions`` or ``switch_cost``, which then stands for the matrix ``-switch_cost (1 - I)``; ``smooth``
        1): the labels stay the path's, and ``conf`` - so ``score`` and ``peak`` - is the posterior probability of the label given
        every position of its video under the same HMM (forward-backward, ``tn_event_decoder_run_posteriors``; on the host
        ``events.hmm_posteriors``).  ``return_posteriors`` implies it and adds ``posterior`` (M, C) float32.  False: the call is what
        it was."""
        posteriors = bool(posteriors or return_posteriors)
        if posteriors:                                                          # refused before anything is launched
            if int(smooth) != 1:
                raise ValueError(f"EventDecoder.decode: posteriors score a path of the unsmoothed scores, not together with smooth={smooth}")
            if transitions is None and switch_cost is None:
                raise ValueError("EventDecoder.decode: posteriors are those of the path's HMM, give transitions or switch_cost")
        if transitions is not None:                                             # refused before anything is launched
            if int(smooth) != 1:
                raise ValueError(f"EventDecoder.decode: transitions decodes the unsmoothed scores, not together with smooth={smooth}")
            if switch_cost is not None:
                raise ValueError(f"EventDecoder.decode: transitions is a matrix of switch costs, not together with switch_cost={switch_cost}")
            if isinstance(transitions, torch.Tensor):
                if transitions.device.type != "cpu":
                    raise ValueError(f"EventDecoder.decode: transitions is read on the host, got a tensor on {transitions.device}")
                transitions = transitions.detach().numpy()
            from .events import check_transitions
            transitions = np.ascontiguousarray(check_transitions(transitions, logits.shape[-1], "EventDecoder.decode"))
        if switch_cost is not None:                                             # refused before anything is launched
            if int(smooth) != 1:
                raise ValueError(f"EventDecoder.decode: switch_cost decodes the unsmoothed scores, not together with smooth={smooth}")
            switch_cost = float(switch_cost)
            if not (np.isfinite(switch_cost) and switch_cost >= 0):
                raise ValueError(f"EventDecoder.decode: switch_cost must be finite and >= 0, got {switch_cost}")
            if posteriors and transitions is None:
                c = int(logits.shape[-1])
                transitions = np.ascontiguousarray(-np.float32(switch_cost) * (1 - np.eye(c, dtype=np.float32)))
        _on_ctx_device(self.ctx, logits, "EventDecoder.decode")
        if logits.dim() != 2 or logits.dtype != torch.float32:
            raise ValueError(f"EventDecoder.decode: logits must be (N, C) float32, got {tuple(logits.shape)} {logits.dtype}")
        logits = logits.contiguous()
        rows, start = _index_arrays(logits.device, rows, start)
        m, dev = rows.shape[0], logits.device
        ints = torch.empty((3, max(m, 1)), dtype=torch.int32, device=dev)
        flts = torch.empty((2, max(m, 1)), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        label = torch.empty(m, dtype=torch.int32, device=dev) if return_frames else None
        conf = torch.empty(m, dtype=torch.float32, device=dev) if return_frames else None
        post = torch.empty((m, logits.shape[1]), dtype=torch.float32, device=dev) if return_posteriors else None
        # the entries differ in one argument, between the positions and the outputs (and the posteriors' in one output more)
        more = ()
        if posteriors:
            entry, how, more = "tn_event_decoder_run_posteriors", transitions.ctypes.data_as(C.c_void_p), (ptr(post),)
        elif transitions is not None:
            entry, how = "tn_event_decoder_run_transitions", transitions.ctypes.data_as(C.c_void_p)
        elif switch_cost is not None:
            entry, how = "tn_event_decoder_run_switch", switch_cost
        else:
            entry, how = "tn_event_decoder_run", int(smooth)
        check(getattr(self.lib, entry)(self.handle, ptr(logits), logits.shape[0], logits.shape[1], ptr(rows), ptr(start), m, how, ptr(label),
                                       ptr(conf), *more, ptr(ints[0]), ptr(ints[1]), ptr(ints[2]), ptr(flts[0]), ptr(flts[1]), ptr(count), None),
              entry)                                                             # (stream NULL: the context's)
        k = int(count.item())
        out = dict(first=ints[0, :k], last=ints[1, :k], cls=ints[2, :k], score=flts[0, :k], peak=flts[1, :k])
        if return_frames:
            out.update(label=label, conf=conf)
        if return_posteriors:
            out["posterior"] = post
        return out



class BiRNN(_Handle):
    """``mx.gluon.rnn.GRU/LSTM(hidden, layout='NTC', bidirectional=...)`` (definitions.py:94-96)."""

    _ABI = "tn_birnn"

    def __init__(self, mode: str, input_size: int, hidden: int, params: dict, prefix: str,
                 bidirectional: bool = True, max_rows: int = 4096, ctx: _lib.Context | None = None):
        super().__init__(ctx)
        self.mode, self.hidden, self.input_size = mode, hidden, input_size
        self.dirs = 2 if bidirectional else 1
        self.max_rows = max_rows
        arr, keep = _lib.make_params({k: v for k, v in params.items() if k.startswith(prefix)})
        h = C.c_void_p()
        kind = _lib.RNN_GRU if mode == "gru" else _lib.RNN_LSTM
        check(self.lib.tn_birnn_create(self.ctx.handle, kind, input_size, hidden, arr, len(arr), prefix.encode(),
                                       1 if bidirectional else 0, max_rows, C.byref(h)), "tn_birnn_create")
        del keep
        self.handle = h

    def __call__(self, x: torch.Tensor, valid_length: torch.Tensor | None = None, return_state: bool = False):
        _on_ctx_device(self.ctx, x, "BiRNN")
        x = x.contiguous().float()
        b, t, f = x.shape
        if f != self.input_size:
            raise ValueError(f"rnn expects {self.input_size} input features, got {f}")
        seq = torch.empty((b, t, self.dirs * self.hidden), dtype=torch.float32, device=x.device)
        hl = torch.empty((self.dirs, b, self.hidden), dtype=torch.float32, device=x.device)
        cl = torch.zeros_like(hl)
        vl = None if valid_length is None else valid_length.to(device=x.device, dtype=torch.int32).contiguous()
        check(self.lib.tn_birnn_forward(self.handle, ptr(x), b, t, ptr(vl), ptr(seq), ptr(hl), ptr(cl)),
              "tn_birnn_forward")
        return (seq, hl, cl) if return_state else seq



def _max_only(kind: str, what: str):
    if kind != "max":
        raise ValueError(f"{what}(..., return_steps=True) is for the max pool: a mean is read from every step alike")


def temporal_pool(x: torch.Tensor, kind: str, ctx: _lib.Context | None = None, return_steps: bool = False):
    """``F.max(x, axis=1)`` / ``F.mean(x, axis=1)`` (definitions.py:66-69,107).  ``return_steps=True`` (max only): ``(y, steps)``,
    ``steps`` int32 of ``y``'s shape, the first position along axis 1 that holds each maximum."""
    ctx = ctx or _lib.default_context(x.device.index)
    x = x.contiguous().float()
    b, t = x.shape[:2]
    f = int(np.prod(x.shape[2:]))
    y = torch.empty((b,) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    if return_steps:
        _max_only(kind, "temporal_pool")
        arg = torch.empty(y.shape, dtype=torch.int32, device=x.device)
        check(ctx.lib.tn_temporal_pool_arg(ctx.handle, ptr(x), b, t, f, ptr(y), ptr(arg)), "tn_temporal_pool_arg")
        return y, arg
    check(ctx.lib.tn_temporal_pool(ctx.handle, ptr(x), b, t, f, _lib.POOL_MEAN if kind == "mean" else _lib.POOL_MAX,
                                   ptr(y)), "tn_temporal_pool")
    return y


def _index_arrays(dev, *arrays):
    """(samples,) index arrays (numpy / torch, any integer type) -> contiguous int32 tensors on ``dev``"""
    out = []
    for a in arrays:
        a = torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a)
        out.append(a.to(device=dev, dtype=torch.int32).contiguous())
    if len({tuple(a.shape) for a in out}) != 1 or out[0].dim() != 1:
        raise ValueError("centre, lo and hi must be one-dimensional arrays of one length")
    return out


def _index_table(dev, idx):
    """a (samples, window) row table (numpy / torch, any integer type) -> a contiguous int32 tensor on ``dev``"""
    idx = torch.as_tensor(np.asarray(idx) if not isinstance(idx, torch.Tensor) else idx)
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError(f"the row table must be a non-empty (samples, window) array, got {tuple(idx.shape)}")
    return idx.to(device=dev, dtype=torch.int32).contiguous()


class WindowHead(_Handle):
    """Dense windowed evaluation of ``CNNRNN`` in feature mode (reference evaluate.py:274-303 with ``--feats_model M --window W
    --temp_pool gru|lstm``; definitions.py:94-96,106-109): ``project`` runs the i2h projection once per row of a device-resident
    (rows, F) feature matrix, ``forward`` gathers every sample's window inside the recurrent kernel - step ``t`` of sample ``b`` reads
    row ``clamp(centre[b] + (t - window // 2) * stride, lo[b], hi[b])`` (``TennisSet.window_rows``) - and returns the logits.  One
    ``project`` serves any number of ``forward`` calls; neither allocates in the library."""

    _ABI = "tn_window_head"

    def __init__(self, mode: str, input_size: int, hidden: int, classes: int, params: dict, rnn_prefix: str, dense_prefix: str,
                 max_rows: int = 65536, max_samples: int | None = None, ctx: _lib.Context | None = None):
        if mode not in ("gru", "lstm"):
            raise ValueError(f"mode must be 'gru' or 'lstm', got {mode!r}")
        super().__init__(ctx)
        self.mode, self.input_size, self.hidden, self.classes = mode, input_size, hidden, classes
        self.max_rows = int(max_rows)
        self.max_samples = int(max_rows if max_samples is None else max_samples)
        arr, keep = _lib.make_params({k: v for k, v in params.items() if k.startswith(rnn_prefix) or k.startswith(dense_prefix)})
        h = C.c_void_p()
        check(self.lib.tn_window_head_create(self.ctx.handle, _lib.RNN_GRU if mode == "gru" else _lib.RNN_LSTM, input_size, hidden,
                                             classes, arr, len(arr), rnn_prefix.encode(), dense_prefix.encode(), self.max_rows,
                                             self.max_samples, C.byref(h)), "tn_window_head_create")
        del keep
        self.handle = h
        self.rows = 0

    def project(self, features: torch.Tensor):
        _on_ctx_device(self.ctx, features, "WindowHead.project")
        x = features.contiguous().float()
        if x.dim() != 2 or x.shape[1] != self.input_size:
            raise ValueError(f"WindowHead expects a (rows, {self.input_size}) feature matrix, got {tuple(x.shape)}")
        self.rows = 0
        check(self.lib.tn_window_head_project(self.handle, ptr(x), x.shape[0]), "tn_window_head_project")
        self.rows = x.shape[0]
        return self

    def forward(self, centre, lo, hi, window: int, stride: int = 1, return_pooled: bool = False, return_tam: bool = False,
                return_steps: bool = False):
        """``return_tam=True``: ``(logits, tam)`` - ``(logits, pooled, tam)`` with ``return_pooled`` - with ``tam`` (samples,
        classes, window) the temporal activation maps (``Dense.step_maps``): ``bias[c] + tam[b, c].sum()`` is ``logits[b, c]``.
        ``return_steps`` appends ``steps`` (samples, 2H) int32, the window position each pooled unit was read from.  ``logits`` and
        ``pooled`` are the bits of the call without maps."""
        dev = torch.device("cuda", self.ctx.device)
        centre, lo, hi = _index_arrays(dev, centre, lo, hi)
        n = centre.shape[0]
        logits = torch.empty((n, self.classes), dtype=torch.float32, device=dev)
        pooled = torch.empty((n, 2 * self.hidden), dtype=torch.float32, device=dev) if return_pooled else None
        if return_tam or return_steps:
            steps = torch.empty((n, 2 * self.hidden), dtype=torch.int32, device=dev) if return_steps else None
            tam = torch.empty((n, self.classes, int(window)), dtype=torch.float32, device=dev)
            check(self.lib.tn_window_head_forward_tam(self.handle, ptr(centre), ptr(lo), ptr(hi), n, int(window), int(stride),
                                                      ptr(pooled), ptr(logits), ptr(steps), ptr(tam)), "tn_window_head_forward_tam")
            return self._with_maps(logits, pooled, tam, steps, return_tam)
        check(self.lib.tn_window_head_forward(self.handle, ptr(centre), ptr(lo), ptr(hi), n, int(window), int(stride), ptr(pooled),
                                              ptr(logits)), "tn_window_head_forward")
        return (logits, pooled) if return_pooled else logits

    __call__ = forward

    @staticmethod
    def _with_maps(logits, pooled, tam, steps, return_tam):
        out = (logits,) + (() if pooled is None else (pooled,)) + ((tam,) if return_tam else ()) + (() if steps is None else (steps,))
        return out

    def forward_rows(self, idx, return_pooled: bool = False, return_tam: bool = False, return_steps: bool = False):
        """``forward`` over a row table (``TennisSet.window_table``): ``idx`` (samples, window) integers, step ``t`` of sample ``b``
        reads row ``clamp(idx[b, t], 0, rows - 1)`` of the projected matrix (a negative entry is row 0).  Any sample layout; a table
        that spells out a ``(centre, lo, hi, stride)`` window gives ``forward``'s bits, ``return_tam`` / ``return_steps`` included."""
        dev = torch.device("cuda", self.ctx.device)
        idx = _index_table(dev, idx)
        n, window = idx.shape
        logits = torch.empty((n, self.classes), dtype=torch.float32, device=dev)
        pooled = torch.empty((n, 2 * self.hidden), dtype=torch.float32, device=dev) if return_pooled else None
        if return_tam or return_steps:
            steps = torch.empty((n, 2 * self.hidden), dtype=torch.int32, device=dev) if return_steps else None
            tam = torch.empty((n, self.classes, window), dtype=torch.float32, device=dev)
            check(self.lib.tn_window_head_forward_rows_tam(self.handle, ptr(idx), n, window, ptr(pooled), ptr(logits), ptr(steps),
                                                           ptr(tam)), "tn_window_head_forward_rows_tam")
            return self._with_maps(logits, pooled, tam, steps, return_tam)
        check(self.lib.tn_window_head_forward_rows(self.handle, ptr(idx), n, window, ptr(pooled), ptr(logits)),
              "tn_window_head_forward_rows")
        return (logits, pooled) if return_pooled else logits

    def _set_rows_per_group(self, nb: int):
        """tuning hook (scripts/bench_window_head.py): samples per workgroup of the recurrent kernel, 0 = the library's choice"""
        check(self.lib.tn_dbg_window_head_rows_per_group(self.handle, int(nb)), "tn_dbg_window_head_rows_per_group")



def temporal_pool_windows(features: torch.Tensor, centre, lo, hi, window: int, stride: int, kind: str,
                          ctx: _lib.Context | None = None, return_steps: bool = False):
    """``F.max`` / ``F.mean`` over axis 1 of the windows of a (rows, F) feature matrix without materialising them
    (definitions.py:66-69 on the batch of dataset.py:190-213) -> (samples, F).  ``return_steps=True`` (max only): ``(y, steps)``,
    ``steps`` (samples, F) int32 the first window position whose row holds the maximum."""
    ctx = ctx or _lib.default_context(features.device.index)
    _on_ctx_device(ctx, features, "temporal_pool_windows")
    x = features.contiguous().float()
    if x.dim() != 2:
        raise ValueError(f"temporal_pool_windows expects a (rows, F) feature matrix, got {tuple(x.shape)}")
    centre, lo, hi = _index_arrays(x.device, centre, lo, hi)
    n = centre.shape[0]
    y = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
    if return_steps:
        _max_only(kind, "temporal_pool_windows")
        arg = torch.empty(y.shape, dtype=torch.int32, device=x.device)
        check(ctx.lib.tn_temporal_pool_windows_arg(ctx.handle, ptr(x), x.shape[0], x.shape[1], ptr(centre), ptr(lo), ptr(hi), n,
                                                   int(window), int(stride), ptr(y), ptr(arg)), "tn_temporal_pool_windows_arg")
        return y, arg
    check(ctx.lib.tn_temporal_pool_windows(ctx.handle, ptr(x), x.shape[0], x.shape[1], ptr(centre), ptr(lo), ptr(hi), n, int(window),
                                           int(stride), _lib.POOL_MEAN if kind == "mean" else _lib.POOL_MAX, ptr(y)),
          "tn_temporal_pool_windows")
    return y


def temporal_pool_rows(features: torch.Tensor, idx, kind: str, ctx: _lib.Context | None = None, return_steps: bool = False):
    """``temporal_pool_windows`` over a row table (``TennisSet.window_table``): sample ``b`` pools the rows
    ``clamp(idx[b, t], 0, rows - 1)``, t ascending -> (samples, F); ``return_steps`` as there."""
    ctx = ctx or _lib.default_context(features.device.index)
    _on_ctx_device(ctx, features, "temporal_pool_rows")
    x = features.contiguous().float()
    if x.dim() != 2:
        raise ValueError(f"temporal_pool_rows expects a (rows, F) feature matrix, got {tuple(x.shape)}")
    idx = _index_table(x.device, idx)
    n, window = idx.shape
    y = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
    if return_steps:
        _max_only(kind, "temporal_pool_rows")
        arg = torch.empty(y.shape, dtype=torch.int32, device=x.device)
        check(ctx.lib.tn_temporal_pool_rows_arg(ctx.handle, ptr(x), x.shape[0], x.shape[1], ptr(idx), n, window, ptr(y), ptr(arg)),
              "tn_temporal_pool_rows_arg")
        return y, arg
    check(ctx.lib.tn_temporal_pool_rows(ctx.handle, ptr(x), x.shape[0], x.shape[1], ptr(idx), n, window,
                                        _lib.POOL_MEAN if kind == "mean" else _lib.POOL_MAX, ptr(y)), "tn_temporal_pool_rows")
    return y


def to_tensor_normalize(x: torch.Tensor, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                        ctx: _lib.Context | None = None) -> torch.Tensor:
    """``transforms.ToTensor()`` + ``transforms.Normalize(mean, std)`` (reference evaluate.py:96-97) on a uint8
    (..., H, W, 3) device batch -> float32 of the same (NHWC) shape."""
    ctx = ctx or _lib.default_context(x.device.index)
    _on_ctx_device(ctx, x, "to_tensor_normalize")
    if x.dtype != torch.uint8 or x.shape[-1] != 3:
        raise ValueError(f"expected uint8 (..., H, W, 3) frames, got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    sd = (C.c_float * 3)(*[float(v) for v in std])
    check(ctx.lib.tn_to_tensor_normalize(ctx.handle, ptr(x), x.numel() // 3, m, sd, ptr(y)), "tn_to_tensor_normalize")
    return y


class GNMTCaptioner(_Handle):
    """Encoder + attention decoder + beam search of the reference captioner on the GPU
    (train_gnmt.py:223-252 assembly; evaluate() at train_gnmt.py:264-302)."""

    _ABI = "tn_gnmt"

    def __init__(self, params: dict, input_size: int, hidden: int, embed: int, vocab: int, beam: int = 4,
                 max_length: int = 150, max_batch: int = 32, max_src_len: int = 640, prefix: str = "gnmt_",
                 cell_type: str = "gru", num_layers: int = 2, num_bi_layers: int = 1, use_residual: bool = False,
                 ctx: _lib.Context | None = None):
        """``num_layers`` / ``num_bi_layers`` / ``use_residual`` as in ``get_gnmt_encoder_decoder`` (reference gnmt.py:407-455):
        2 <= num_layers, num_bi_layers < num_layers (gnmt.py:78-80 and the attention's key width, see tn_gnmt_create_ex)."""
        super().__init__(ctx)
        self.hidden, self.beam, self.max_length, self.vocab, self.input_size = hidden, beam, max_length, vocab, input_size
        arr, keep = _lib.make_params({k: v for k, v in params.items() if k.startswith(prefix)})
        h = C.c_void_p()
        kind = _lib.RNN_GRU if cell_type == "gru" else _lib.RNN_LSTM
        check(self.lib.tn_gnmt_create_ex(self.ctx.handle, arr, len(arr), prefix.encode(), kind, input_size, hidden, embed,
                                         vocab, num_layers, num_bi_layers, max_batch, max_src_len, beam, max_length,
                                         1 if use_residual else 0, C.byref(h)), "tn_gnmt_create")
        del keep
        self.handle = h
        self._batch = self._steps = 0

    def encode(self, src: torch.Tensor, valid_length: torch.Tensor) -> torch.Tensor:
        src = src.contiguous().float()
        b, t, _ = src.shape
        vl = valid_length.to(device=src.device).round().to(torch.int32).contiguous()
        mem = torch.empty((b, t, self.hidden), dtype=torch.float32, device=src.device)
        check(self.lib.tn_gnmt_encode(self.handle, ptr(src), ptr(vl), b, t, ptr(mem)), "tn_gnmt_encode")
        self._batch, self._steps = b, t
        return mem

    def encode_rows(self, table: torch.Tensor, idx, valid_length) -> torch.Tensor:
        """``encode(pad(table[idx]), valid_length)`` without the (B, T, F) batch: ``idx`` (B, T) names each step's row of the
        device-resident ``table`` (rows, F), -1 behind a clip's end (a row of zeros); encoder layer 0's i2h product gathers the rows
        while it stages them, in the same arithmetic order: ``mem`` and everything ``decode_seq`` / ``beam_search`` derive from it are
        bit-identical to the materialised route."""
        table = _clip_table(self.ctx, table, self.input_size, "encode_rows")
        idx = _clip_rows(self.ctx, table, idx, valid_length, "encode_rows")
        b, t = idx.shape
        vl = torch.as_tensor(valid_length).to(device=table.device).round().to(torch.int32).contiguous()
        mem = torch.empty((b, t, self.hidden), dtype=torch.float32, device=table.device)
        check(self.lib.tn_gnmt_encode_rows(self.handle, ptr(table), table.shape[0], table.stride(0), ptr(idx), ptr(vl), b, t, ptr(mem)),
              "tn_gnmt_encode_rows")
        self._batch, self._steps = b, t
        return mem

    def decode_seq(self, tgt: torch.Tensor, return_attention: bool = False):
        """Teacher-forced logits (B, L, V) for target tokens (B, L) after encode().  ``return_attention``: ``(logits, attention)``
        with the decoder's attention weights (B, L, T) over the T encoder steps of the last ``encode`` / ``encode_rows`` (what
        ``GNMTDecoder(output_attention=True).decode_seq`` stacks, reference gnmt.py:302-303), zeros at and beyond a clip's
        ``valid_length``."""
        tgt = tgt.to(device=torch.device("cuda", self.ctx.device)).round().to(torch.int32).contiguous()
        b, l = tgt.shape
        logits = torch.empty((b, l, self.vocab), dtype=torch.float32, device=tgt.device)
        if return_attention:
            att = torch.empty((b, l, self._steps), dtype=torch.float32, device=tgt.device)
            check(self.lib.tn_gnmt_decode_seq_attention(self.handle, ptr(tgt), l, l, ptr(logits), ptr(att)),
                  "tn_gnmt_decode_seq_attention")
            return logits, att
        check(self.lib.tn_gnmt_decode_seq(self.handle, ptr(tgt), l, l, ptr(logits)), "tn_gnmt_decode_seq")
        return logits

    def beam_search(self, bos: int, eos: int, alpha: float = 1.0, K: float = 5.0, max_length: int | None = None,
                    return_attention: bool = False):
        """``(samples (B, beam, n), scores, valid_length)``; with ``return_attention`` a fourth tensor ``attention (B, beam, n - 1, T)``:
        row ``i`` of a hypothesis holds the weights of the decoder step that emitted its token ``i + 1``, followed through the
        beam reshuffling, zeros where no step emitted the token (the ``-1`` padding, an ``<eos>`` appended at ``max_length``)."""
        ml = self.max_length if max_length is None else max_length
        b, dev = self._batch, torch.device("cuda", self.ctx.device)
        samples = torch.empty((b, self.beam, self.max_length + 2), dtype=torch.int32, device=dev)
        scores = torch.empty((b, self.beam), dtype=torch.float32, device=dev)
        vlen = torch.empty((b, self.beam), dtype=torch.int32, device=dev)
        n = C.c_int(0)
        if return_attention:
            att = torch.empty((b, self.beam, self.max_length + 1, max(self._steps, 1)), dtype=torch.float32, device=dev)
            check(self.lib.tn_gnmt_beam_search_attention(self.handle, bos, eos, alpha, K, ml, ptr(samples), ptr(scores), ptr(vlen),
                                                         C.byref(n), ptr(att)), "tn_gnmt_beam_search_attention")
            return samples[:, :, :n.value].contiguous(), scores, vlen, att[:, :, :n.value - 1].contiguous()
        check(self.lib.tn_gnmt_beam_search(self.handle, bos, eos, alpha, K, ml, ptr(samples), ptr(scores), ptr(vlen),
                                           C.byref(n)), "tn_gnmt_beam_search")
        return samples[:, :, :n.value].contiguous(), scores, vlen



def masked_softmax_ce(logits: torch.Tensor, labels: torch.Tensor, valid_length: torch.Tensor,
                      ctx: _lib.Context | None = None) -> torch.Tensor:
    """``gluonnlp.loss.MaskedSoftmaxCELoss`` (reference train_gnmt.py:256,281): (B,) losses."""
    ctx = ctx or _lib.default_context(logits.device.index)
    logits = logits.contiguous().float()
    b, l, v = logits.shape
    lab = labels.to(logits.device).round().to(torch.int32).contiguous()
    vl = valid_length.to(logits.device).round().to(torch.int32).contiguous()
    loss = torch.empty((b,), dtype=torch.float32, device=logits.device)
    check(ctx.lib.tn_masked_softmax_ce(ctx.handle, ptr(logits), ptr(lab), lab.shape[1], ptr(vl), b, l, v, ptr(loss)),
          "tn_masked_softmax_ce")
    return loss


class TemporalHeadTrainer(_FlatTrainer):
    """Training step of ``CNNRNN(model=None, type='gru' | 'lstm')`` in feature mode (reference definitions.py:94-110) the way
    train.py drives it: ``SoftmaxCrossEntropyLoss`` per sample (:324), ``ag.backward`` of the per-sample losses and
    ``gluon.Trainer(params, 'sgd', {learning_rate, momentum, wd}).step(batch_size)`` (:298-299, :410-424).

    ``forward_backward`` leaves the gradient of the SUM of the per-sample losses in a flat device buffer
    (``grads``); with several ranks all-reduce that buffer (``torch.distributed.all_reduce(trainer.grads)``)
    before ``step(batch_size)``, whose ``rescale_grad = 1 / batch_size`` is Gluon's."""
    _ABI = "tn_head"

    def __init__(self, params: dict, input_size: int, hidden: int = 128, classes: int = 11, max_batch: int = 32,
                 max_steps: int = 64, rnn_prefix: str | None = None, dense_prefix: str = "cnnrnn0_dense0_",
                 ctx: _lib.Context | None = None, type: str = "gru"):
        if type not in ("gru", "lstm"):
            raise ValueError(f"type must be 'gru' or 'lstm', got {type!r}")
        if rnn_prefix is None:
            rnn_prefix = f"cnnrnn0_{type}0_"
        self.type, self.gates = type, 3 if type == "gru" else 4
        super().__init__(ctx)
        self.input_size, self.hidden, self.classes = input_size, hidden, classes
        self.rnn_prefix, self.dense_prefix = rnn_prefix, dense_prefix
        arr, keep = self._select(params, rnn_prefix, dense_prefix)
        h = C.c_void_p()
        check(self.lib.tn_head_create(self.ctx.handle, _lib.RNN_GRU if type == "gru" else _lib.RNN_LSTM, input_size, hidden, classes, arr, len(arr), rnn_prefix.encode(),
                                      dense_prefix.encode(), max_batch, max_steps, C.byref(h)), "tn_head_create")
        del keep
        self._adopt(h)

    def forward_backward(self, x: torch.Tensor, labels: torch.Tensor):
        x = x.contiguous().float()
        b, t, f = x.shape
        labels = labels.to(device=x.device, dtype=torch.int32).contiguous()
        loss = torch.empty((b,), dtype=torch.float32, device=x.device)
        logits = torch.empty((b, self.classes), dtype=torch.float32, device=x.device)
        check(self.lib.tn_head_forward_backward(self.handle, ptr(x), ptr(labels), b, t, ptr(loss), ptr(logits)),
              "tn_head_forward_backward")
        return loss, logits

    def set_features(self, table: torch.Tensor):
        """The (rows, F) fp32 feature table the ``*_rows`` calls gather their windows from.  It has to be on the handle's GPU already
        (uploaded once); the library borrows it, so the trainer keeps the tensor alive."""
        _on_ctx_device(self.ctx, table, "TemporalHeadTrainer.set_features")
        if table.dim() != 2 or table.shape[1] != self.input_size or table.shape[0] < 1 or table.dtype != torch.float32:
            raise ValueError(f"set_features: need a (rows, {self.input_size}) float32 table, got {tuple(table.shape)} {table.dtype}")
        table = table.contiguous()
        check(self.lib.tn_head_set_features(self.handle, ptr(table), table.shape[0], table.stride(0)), "tn_head_set_features")
        self._features = table

    def _row_idx(self, idx, what: str) -> torch.Tensor:
        """(B, T) window rows -> int32 on the handle's GPU.  A host-side ``idx`` (numpy array, CPU tensor, nested list) is
        range-checked here, before any launch; a device tensor is passed through and the kernels clamp."""
        table = getattr(self, "_features", None)
        if table is None:
            raise RuntimeError(f"{what}: no feature table (call set_features first)")
        if isinstance(idx, torch.Tensor) and idx.is_cuda:
            _on_ctx_device(self.ctx, idx, what)
        else:
            host = idx.numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
            if host.dtype.kind not in "iu":
                raise ValueError(f"{what}: idx must hold integers, got {host.dtype}")
            if host.size and (int(host.min()) < 0 or int(host.max()) >= table.shape[0]):
                raise ValueError(f"{what}: idx must lie in [0, {table.shape[0] - 1}], got [{int(host.min())}, {int(host.max())}]")
            idx = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(table.device)
        if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise ValueError(f"{what}: idx must be (batch, steps), got {tuple(idx.shape)}")
        return idx.to(torch.int32).contiguous()

    def forward_backward_rows(self, idx, labels: torch.Tensor):
        """``forward_backward(table[idx], labels)`` without the (B, T, F) batch: ``idx`` (B, T) names each window step's row of the
        table given to ``set_features``; the kernels gather the rows while they stage them, in the same arithmetic order, so loss,
        logits and gradients are bit-identical to the materialised step."""
        idx = self._row_idx(idx, "forward_backward_rows")
        b, t = idx.shape
        labels = labels.to(device=idx.device, dtype=torch.int32).contiguous()
        loss = torch.empty((b,), dtype=torch.float32, device=idx.device)
        logits = torch.empty((b, self.classes), dtype=torch.float32, device=idx.device)
        check(self.lib.tn_head_forward_backward_rows(self.handle, ptr(idx), ptr(labels), b, t, ptr(loss), ptr(logits)),
              "tn_head_forward_backward_rows")
        return loss, logits

    def predict_rows(self, idx) -> torch.Tensor:
        """The forward half of ``forward_backward_rows``: (B, classes) logits of the current parameters; gradients, momentum and
        parameters are untouched."""
        idx = self._row_idx(idx, "predict_rows")
        b, t = idx.shape
        logits = torch.empty((b, self.classes), dtype=torch.float32, device=idx.device)
        check(self.lib.tn_head_forward_rows(self.handle, ptr(idx), b, t, ptr(logits)), "tn_head_forward_rows")
        return logits

    def step(self, batch_size: int, lr: float, momentum: float = 0.9, wd: float = 1e-4):
        check(self.lib.tn_head_sgd_step(self.handle, lr, momentum, wd, 1.0 / batch_size), "tn_head_sgd_step")

    def get(self, name: str, gradient: bool = False, shape=None) -> np.ndarray:
        """A name without a recorded shape is read flat (no parameter is larger than the flat buffer); an unknown one raises the
        library's error."""
        return super().get(name, gradient, shape or self.shapes.get(name) or (self.numel,))


class GNMTTrainer(_FlatTrainer):
    """One training step of the captioner the way reference train_gnmt.py::train drives it (:328-337): teacher-forced
    ``NMTModel`` forward, token-averaged ``MaskedSoftmaxCELoss``, ``loss.backward()``, ``gluon.Trainer('adam').step(1)``.
    GRU (the reference's flag default) or LSTM cells; ``num_layers`` / ``num_bi_layers`` / ``use_residual`` as the reference's
    flags pass them into the model it trains (train_gnmt.py:58-61,223-227; round 4: any ``num_layers >= 2`` with
    ``num_bi_layers < num_layers``).  ``grads`` / ``params`` are flat device views for a data-parallel all-reduce between
    ``forward_backward`` and ``step``."""
    _ABI = "tn_gnmt_trainer"

    def __init__(self, params: dict, input_size: int, hidden: int, embed: int, vocab: int, max_batch: int = 32,
                 max_src_len: int = 256, max_tgt_len: int = 64, prefix: str = "gnmt_", ctx: _lib.Context | None = None,
                 cell_type: str = "gru", num_layers: int = 2, num_bi_layers: int = 1, use_residual: bool = False):
        if cell_type not in ("gru", "lstm"):
            raise ValueError(f"cell_type must be 'gru' or 'lstm', got {cell_type!r}")
        self.num_layers, self.num_bi_layers, self.use_residual = num_layers, num_bi_layers, bool(use_residual)
        super().__init__(ctx)
        self.input_size, self.hidden, self.embed, self.vocab, self.prefix = input_size, hidden, embed, vocab, prefix
        self.cell_type = cell_type
        arr, keep = self._select(params, prefix)
        h = C.c_void_p()
        check(self.lib.tn_gnmt_trainer_create_ex(self.ctx.handle, arr, len(arr), prefix.encode(),
                                                 _lib.RNN_GRU if cell_type == "gru" else _lib.RNN_LSTM, input_size, hidden, embed, vocab,
                                                 num_layers, num_bi_layers, 1 if use_residual else 0,
                                                 max_batch, max_src_len, max_tgt_len, C.byref(h)), "tn_gnmt_trainer_create_ex")
        del keep
        self._adopt(h)

    def forward_backward(self, src: torch.Tensor, src_valid_length: torch.Tensor, tgt: torch.Tensor,
                         tgt_valid_length: torch.Tensor, return_logits: bool = False):
        """src (B,T,F) fp32, tgt (B,L) token ids incl. BOS / EOS, valid lengths (B,) -> loss (0-d tensor) [, logits (B,L-1,V)]"""
        src = src.contiguous().float()
        b, t, _ = src.shape
        dev = src.device
        tgt = tgt.to(device=dev, dtype=torch.int32).contiguous()
        svl = src_valid_length.to(device=dev, dtype=torch.int32).contiguous()
        tvl = tgt_valid_length.to(device=dev, dtype=torch.int32).contiguous()
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        logits = torch.empty((b, tgt.shape[1] - 1, self.vocab), dtype=torch.float32, device=dev) if return_logits else None
        check(self.lib.tn_gnmt_trainer_forward_backward(self.handle, ptr(src), ptr(svl), ptr(tgt), tgt.shape[1], ptr(tvl), b, t,
                                                        tgt.shape[1], ptr(loss), ptr(logits)), "tn_gnmt_trainer_forward_backward")
        return (loss[0], logits) if return_logits else loss[0]

    def forward_backward_rows(self, table: torch.Tensor, idx, src_valid_length, tgt: torch.Tensor, tgt_valid_length,
                              return_logits: bool = False):
        """``forward_backward(pad(table[idx]), ...)`` without the (B, T, F) batch: ``table`` (rows, F) fp32 lives on the GPU (uploaded
        once per split), ``idx`` (B, T) names each step's row, -1 behind a clip's end (the zero padding of the materialised batch).
        Layer 0's i2h product and dW_ih gather the rows while they stage them, in the same arithmetic order: loss, logits and
        gradients are bit-identical to the materialised step."""
        table = _clip_table(self.ctx, table, self.input_size, "forward_backward_rows")
        idx = _clip_rows(self.ctx, table, idx, src_valid_length, "forward_backward_rows")
        b, t = idx.shape
        dev = table.device
        tgt = torch.as_tensor(tgt).to(device=dev, dtype=torch.int32).contiguous()
        svl = torch.as_tensor(src_valid_length).to(device=dev, dtype=torch.int32).contiguous()
        tvl = torch.as_tensor(tgt_valid_length).to(device=dev, dtype=torch.int32).contiguous()
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        logits = torch.empty((b, tgt.shape[1] - 1, self.vocab), dtype=torch.float32, device=dev) if return_logits else None
        check(self.lib.tn_gnmt_trainer_forward_backward_rows(self.handle, ptr(table), table.shape[0], table.stride(0), ptr(idx), ptr(svl),
                                                             ptr(tgt), tgt.shape[1], ptr(tvl), b, t, tgt.shape[1], ptr(loss), ptr(logits)),
              "tn_gnmt_trainer_forward_backward_rows")
        return (loss[0], logits) if return_logits else loss[0]

    def set_dropout(self, p: float, seed: int = 0):
        """``--dropout`` of train_gnmt.py (default 0.2 there): after each encoder layer and on the top decoder cell's output."""
        check(self.lib.tn_gnmt_trainer_set_dropout(self.handle, p, seed), "tn_gnmt_trainer_set_dropout")

    def dropout_masks(self, batch: int, src_steps: int, tgt_steps: int):
        """The last step's masks as tensors: (B,T,2H), (B,T,H), (L,B,H) (step-major) - for tests against the oracle."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.lib.tn_gnmt_trainer_dropout_masks(self.handle, C.byref(a), C.byref(b), C.byref(c)), "tn_gnmt_trainer_dropout_masks")
        h, view = self.hidden, lambda addr, shape: _device_view(self.ctx, addr.value, shape)
        return view(a, (batch, src_steps, 2 * h)), view(b, (batch, src_steps, h)), view(c, (tgt_steps, batch, h))

    def dropout_mask(self, which: int, shape) -> torch.Tensor:
        """One mask of the last step: ``which`` = encoder layer ``i`` -> (B,T,dirs*H); ``num_layers + j`` -> decoder layer ``j >= 1``,
        (L,B,H) step-major."""
        a = C.c_void_p()
        check(self.lib.tn_gnmt_trainer_dropout_mask(self.handle, which, C.byref(a)), "tn_gnmt_trainer_dropout_mask")
        return _device_view(self.ctx, a.value, shape)

    def step(self, lr: float, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        check(self.lib.tn_gnmt_trainer_adam_step(self.handle, lr, beta1, beta2, epsilon), "tn_gnmt_trainer_adam_step")


class _BackboneMatmul(_FlatTrainer):
    """``matmul`` of the three backbone trainers: which matrix pipe the backbone's GEMMs run on.  ``"f32"`` (the default) is the
    exact-f32 matrix instruction; ``"fp32x3"`` keeps fp32 operands, accumulators and results and forms every product from three
    bf16 terms per operand on the bf16 matrix pipe (csrc/gemm_fp32x3.hip) - the same float64 bars."""

    def set_matmul(self, name: str):
        mode = _lib.matmul_mode(name)
        fn = getattr(self.lib, self._ABI + "_set_matmul")
        check(fn(self.handle, mode), self._ABI + "_set_matmul")
        self.matmul = name

    def matmul_stats(self) -> tuple:
        """Backbone GEMM launches since construction: (f32, fp32x3)"""
        a, b = C.c_int64(), C.c_int64()
        fn = getattr(self.lib, self._ABI + "_matmul_stats")
        check(fn(self.handle, C.byref(a), C.byref(b)), self._ABI + "_matmul_stats")
        return a.value, b.value


class FrameModelTrainer(_BackboneMatmul):
    """End-to-end fine-tuning step of ``FrameModel(DenseNet121.features, classes)`` the way reference train.py drives it
    with an un-frozen backbone: BatchNorm in training mode, ``SoftmaxCrossEntropyLoss`` per sample (:324), backward of the
    summed losses (:419-421), ``gluon.Trainer('sgd', {lr, momentum, wd}).step(batch_size)`` (:298-299,424).  fp32.  The batch
    size is fixed at construction (BatchNorm statistics are per batch)."""
    _ABI = "tn_finetune"

    def __init__(self, params: dict, size: int = 224, classes: int = 11, batch: int = 8, prefix: str = "densenet0_",
                 dense_prefix: str = "framemodel0_dense0_", ctx: _lib.Context | None = None, matmul: str = "f32"):
        _lib.matmul_mode(matmul)                       # a wrong name raises before a context or the library is touched
        super().__init__(ctx)
        self.size, self.classes, self.batch = size, classes, batch
        arr, keep = self._select(params, prefix, dense_prefix)
        h = C.c_void_p()
        check(self.lib.tn_finetune_create(self.ctx.handle, arr, len(arr), prefix.encode(), dense_prefix.encode(), size, size, classes,
                                          batch, C.byref(h)), "tn_finetune_create")
        del keep
        self._adopt(h)
        self.set_matmul(matmul)

    def forward_backward(self, x: torch.Tensor, labels: torch.Tensor):
        """x: frames as NCHW fp32 (the reference layout) or NHWC fp32, normalised; labels (B,) -> (loss (B,), logits (B, classes))"""
        _on_ctx_device(self.ctx, x, "FrameModelTrainer")
        sz = self.size
        if x.dtype == torch.uint8:        # decoded frames out of transforms.Compose: ToTensor + Normalize here
            x = to_tensor_normalize(x, ctx=self.ctx)
        if x.dim() == 4 and tuple(x.shape[1:]) == (3, sz, sz):
            x = x.permute(0, 2, 3, 1)
        if x.dim() != 4 or tuple(x.shape) != (self.batch, sz, sz, 3):
            raise ValueError(f"FrameModelTrainer expects ({self.batch}, 3, {sz}, {sz}) or ({self.batch}, {sz}, {sz}, 3) frames "
                             f"(apply the Resize/CenterCrop transform first), got {tuple(x.shape)}")
        x = x.contiguous().float()
        b = x.shape[0]
        labels = labels.to(device=x.device, dtype=torch.int32).contiguous()
        loss = torch.empty((b,), dtype=torch.float32, device=x.device)
        logits = torch.empty((b, self.classes), dtype=torch.float32, device=x.device)
        check(self.lib.tn_finetune_forward_backward(self.handle, ptr(x), ptr(labels), b, sz, sz, ptr(loss), ptr(logits)),
              "tn_finetune_forward_backward")
        return loss, logits

    def step(self, batch_size: int, lr: float, momentum: float = 0.9, wd: float = 1e-4):
        check(self.lib.tn_finetune_sgd_step(self.handle, lr, momentum, wd, 1.0 / batch_size), "tn_finetune_sgd_step")


class CNNRNNTrainer(_BackboneMatmul):
    """End-to-end training step of ``CNNRNN(FrameModel(DenseNet121.features))`` over ``TimeDistributed`` frames, the way reference
    train.py:197-236 drives it with ``--window > 1 --temp_pool gru|lstm`` and no ``--feats_model``: the backbone's BatchNorms in
    training mode over all batch x steps frames, bi-GRU / bi-LSTM -> max over T -> Dense, ``SoftmaxCrossEntropyLoss`` per sample
    (:324), backward of the summed losses (:419-421) through the head and, unless ``freeze_backbone`` (:231-233), through the
    backbone; ``gluon.Trainer('sgd', {lr, momentum, wd}).step(batch_size)`` (:298-299,424).  fp32.  Batch and steps are fixed at
    construction (BatchNorm statistics are per batch).

    ``grads`` is a tuple of flat device views: (backbone, head), or (head,) with a frozen backbone - what a data-parallel run
    all-reduces before ``step`` (``train.allreduce_and_step``).  A frozen backbone is not updated, but its BatchNorms still
    normalise with batch statistics and update their running statistics (docs/numerics.md)."""
    _PARTS = 2
    _ABI = "tn_cnnrnn_trainer"

    def __init__(self, params: dict, size: int = 224, classes: int = 11, batch: int = 2, steps: int = 8, type: str = "gru",
                 prefix: str = "densenet0_", rnn_prefix: str | None = None, dense_prefix: str = "cnnrnn0_dense0_",
                 freeze_backbone: bool = False, ctx: _lib.Context | None = None, matmul: str = "f32"):
        _lib.matmul_mode(matmul)                       # a wrong name raises before a context or the library is touched
        if type not in ("gru", "lstm"):
            raise ValueError(f"type must be 'gru' or 'lstm', got {type!r}")
        if rnn_prefix is None:
            rnn_prefix = f"cnnrnn0_{type}0_"
        super().__init__(ctx)
        self.type, self.size, self.classes, self.batch, self.steps = type, size, classes, batch, steps
        self.frozen = bool(freeze_backbone)
        self.prefix, self.rnn_prefix, self.dense_prefix = prefix, rnn_prefix, dense_prefix
        arr, keep = self._select(params, prefix, rnn_prefix, dense_prefix)
        h = C.c_void_p()
        check(self.lib.tn_cnnrnn_trainer_create(self.ctx.handle, _lib.RNN_GRU if type == "gru" else _lib.RNN_LSTM, arr, len(arr),
                                                prefix.encode(), rnn_prefix.encode(), dense_prefix.encode(), size, size, classes,
                                                batch, steps, 1 if self.frozen else 0, C.byref(h)), "tn_cnnrnn_trainer_create")
        del keep
        self._adopt(h)
        self.set_matmul(matmul)

    def forward_backward(self, x: torch.Tensor, labels: torch.Tensor):
        """x: (batch, steps) frames, NCHW or NHWC per frame, fp32 normalised or uint8 (ToTensor + Normalize applied here);
        labels (batch,) -> (loss (batch,), logits (batch, classes))"""
        _on_ctx_device(self.ctx, x, "CNNRNNTrainer")
        b, t, sz = self.batch, self.steps, self.size
        if x.dtype == torch.uint8:
            x = to_tensor_normalize(x, ctx=self.ctx)
        if x.dim() == 5 and tuple(x.shape[2:]) == (3, sz, sz):
            x = x.permute(0, 1, 3, 4, 2)
        if x.dim() != 5 or tuple(x.shape) != (b, t, sz, sz, 3):
            raise ValueError(f"CNNRNNTrainer expects ({b}, {t}, 3, {sz}, {sz}) or ({b}, {t}, {sz}, {sz}, 3) frames, got {tuple(x.shape)}")
        x = x.contiguous().float()
        labels = labels.to(device=x.device, dtype=torch.int32).contiguous()
        loss = torch.empty((b,), dtype=torch.float32, device=x.device)
        logits = torch.empty((b, self.classes), dtype=torch.float32, device=x.device)
        check(self.lib.tn_cnnrnn_trainer_forward_backward(self.handle, ptr(x), ptr(labels), b, t, sz, sz, ptr(loss), ptr(logits)),
              "tn_cnnrnn_trainer_forward_backward")
        return loss, logits

    def step(self, batch_size: int, lr: float, momentum: float = 0.9, wd: float = 1e-4):
        check(self.lib.tn_cnnrnn_trainer_sgd_step(self.handle, lr, momentum, wd, 1.0 / batch_size), "tn_cnnrnn_trainer_sgd_step")


class GNMTFramesTrainer(_BackboneMatmul):
    """One frame-mode training step of the captioner, the way reference train_gnmt.py drives it without ``--feats_model``
    (:148-203, 328-337): ``src_embed = TimeDistributed(FrameModel(DenseNet121.features).backbone)`` inside the ``NMTModel``, so the
    backbone runs in training mode over all batch x steps frames of the padded clips and is trained - or, with ``freeze_backbone``
    (:164-166), left alone - by the same ``loss.backward()`` and ``gluon.Trainer('adam').step(1)``.  fp32.

    Any batch ``<= max_batch`` of any clip length ``<= max_src_len`` runs as long as ``batch * steps <= max_frames``.  The frame slots
    behind a clip's valid length are zeroed (``Pad()``, utils/captioning.py:33) whatever the caller left there; they count in the
    BatchNorm batch statistics, as in the reference (docs/numerics.md).

    ``grads`` is a tuple of flat device views: (backbone, captioner), or (captioner,) with a frozen backbone - what a data-parallel
    run all-reduces before ``step``.  A frozen backbone is not updated, but its BatchNorms still normalise with batch statistics
    and update their running statistics (docs/numerics.md)."""
    _PARTS = 2
    _ABI = "tn_gnmt_frames_trainer"

    def __init__(self, params: dict, hidden: int, embed: int, vocab: int, size: int = 224, max_batch: int = 4, max_src_len: int = 16,
                 max_tgt_len: int = 64, max_frames: int | None = None, prefix: str = "gnmt_", backbone_prefix: str = "densenet0_",
                 freeze_backbone: bool = False, ctx: _lib.Context | None = None, cell_type: str = "gru", num_layers: int = 2,
                 num_bi_layers: int = 1, use_residual: bool = False, matmul: str = "f32"):
        _lib.matmul_mode(matmul)                       # a wrong name raises before a context or the library is touched
        if cell_type not in ("gru", "lstm"):
            raise ValueError(f"cell_type must be 'gru' or 'lstm', got {cell_type!r}")
        super().__init__(ctx)
        self.size, self.hidden, self.embed, self.vocab = size, hidden, embed, vocab
        self.max_batch, self.max_src_len = max_batch, max_src_len
        self.max_frames = max_batch * max_src_len if max_frames is None else max_frames
        self.frozen = bool(freeze_backbone)
        self.prefix, self.backbone_prefix, self.cell_type = prefix, backbone_prefix, cell_type
        arr, keep = self._select(params, prefix, backbone_prefix)
        h = C.c_void_p()
        check(self.lib.tn_gnmt_frames_trainer_create(self.ctx.handle, arr, len(arr), backbone_prefix.encode(), prefix.encode(),
                                                     _lib.RNN_GRU if cell_type == "gru" else _lib.RNN_LSTM, hidden, embed, vocab,
                                                     num_layers, num_bi_layers, 1 if use_residual else 0, size, max_batch, max_src_len,
                                                     max_tgt_len, self.max_frames, 1 if self.frozen else 0, C.byref(h)),
              "tn_gnmt_frames_trainer_create")
        del keep
        self._adopt(h)
        self.set_matmul(matmul)

    def forward_backward(self, frames: torch.Tensor, src_valid_length: torch.Tensor, tgt: torch.Tensor,
                         tgt_valid_length: torch.Tensor, return_logits: bool = False):
        """frames (B,T) clips, NCHW or NHWC per frame, fp32 normalised or uint8 (ToTensor + Normalize applied here); tgt (B,L) token
        ids incl. BOS / EOS, valid lengths (B,) -> loss (0-d tensor) [, logits (B,L-1,V)]"""
        _on_ctx_device(self.ctx, frames, "GNMTFramesTrainer")
        sz = self.size
        x = frames
        if x.dtype == torch.uint8:
            x = to_tensor_normalize(x, ctx=self.ctx)
        if x.dim() == 5 and tuple(x.shape[2:]) == (3, sz, sz):
            x = x.permute(0, 1, 3, 4, 2)
        if x.dim() != 5 or tuple(x.shape[2:]) != (sz, sz, 3):
            raise ValueError(f"GNMTFramesTrainer expects (B, T, 3, {sz}, {sz}) or (B, T, {sz}, {sz}, 3) frames, got {tuple(frames.shape)}")
        x = x.contiguous().float()                 # (read only: the handle stages the frames and zeroes the padded slots there)
        b, t = x.shape[0], x.shape[1]
        dev = x.device
        tgt = tgt.to(device=dev, dtype=torch.int32).contiguous()
        svl = src_valid_length.to(device=dev, dtype=torch.int32).contiguous()
        tvl = tgt_valid_length.to(device=dev, dtype=torch.int32).contiguous()
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        logits = torch.empty((b, tgt.shape[1] - 1, self.vocab), dtype=torch.float32, device=dev) if return_logits else None
        check(self.lib.tn_gnmt_frames_trainer_forward_backward(self.handle, ptr(x), ptr(svl), ptr(tgt), tgt.shape[1], ptr(tvl), b, t,
                                                               tgt.shape[1], ptr(loss), ptr(logits)),
              "tn_gnmt_frames_trainer_forward_backward")
        return (loss[0], logits) if return_logits else loss[0]

    def set_dropout(self, p: float, seed: int = 0):
        """``--dropout`` of train_gnmt.py: after each encoder layer and on the decoder cells' outputs (the backbone has none)."""
        check(self.lib.tn_gnmt_frames_trainer_set_dropout(self.handle, p, seed), "tn_gnmt_frames_trainer_set_dropout")

    def step(self, lr: float, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        check(self.lib.tn_gnmt_frames_trainer_adam_step(self.handle, lr, beta1, beta2, epsilon), "tn_gnmt_frames_trainer_adam_step")
