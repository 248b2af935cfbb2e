"""Streaming validation metrics with the state on the device (csrc/seg_eval.hip, oct_seg_eval_update).

A validation loop scores batch after batch; `Metrics.evaluate(y_true, y_pred, classes=C)` reads its counts back per batch and
knows neither a C x C confusion matrix nor ignore_index.  `SegEvaluator` keeps ONE int64 device buffer

    cm[t*C + p] | thick_abs[c] | columns | ignored | invalid | updates            (C*C + C + 4 entries)

which every update() ADDS to with one kernel launch and no host synchronisation; compute() is the only call that reads it.

  ignored   has ignore_index and t == ignore_index: counted there and nowhere else
  invalid   not ignored, t or p outside [0, C): counted there and nowhere else
  cm        every other ("valid") pixel adds 1 to cm[t][p]
  thick_abs per image b, column x and class c: |T - P| with T = #{y : valid, t == c}, P = #{y : valid, p == c} -- the
            per-layer thickness error per A-scan of the layer-segmentation papers; Biomarker_based_metrics.thickness_difference
            (axis 0 = H) of the masks (t == c), (p == c), for all classes in the same pass.  columns += images * W per update.

    ev = SegEvaluator(classes=9, ignore_index=255)
    for x, y in loader:
        ev.update_model(model, x, y)        # or ev.update(y, class_map) / ev.update_logits(y, logits, "nhwc")
    ev.all_reduce()                         # data-parallel validation: one all-reduce of the state
    m = ev.compute()                        # the one synchronisation; m["confusion"], m["dice_coefficient"], m["thickness_error"]

`metrics_from_state` is pure numpy: the formulas are Metrics._formulas (the reference's epsilons, verbatim) on the one-vs-rest
counts that follow from the confusion matrix.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

_LAYOUTS = {"nhwc": L.SEG_NHWC, "nchw": L.SEG_NCHW, L.SEG_NHWC: L.SEG_NHWC, L.SEG_NCHW: L.SEG_NCHW}
_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.bool)


def state_size(classes: int) -> int:
    return classes * classes + classes + L.EVAL_STATE_EXTRA


def _check_config(classes, ignore_index):
    if isinstance(classes, bool) or not isinstance(classes, int):
        raise TypeError(f"classes must be an int, got {type(classes).__name__} {classes!r}")
    if not 1 <= classes <= L.MAX_CLASSES:
        raise ValueError(f"classes must be in 1..{L.MAX_CLASSES} (got {classes})")
    if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)):
        raise TypeError(f"ignore_index must be an int or None, got {type(ignore_index).__name__} {ignore_index!r}")
    if ignore_index is not None and not -2 ** 63 <= ignore_index < 2 ** 63:
        raise ValueError(f"ignore_index {ignore_index} is not an int64")


def metrics_from_state(state, classes: int) -> dict:
    """Every metric of the evaluator from its int64 state (numpy, no GPU): see SegEvaluator.compute."""
    from .Metrics import _formulas
    _check_config(classes, None)
    s = np.asarray(state)
    if s.dtype.kind not in "iu" or s.size != state_size(classes):
        raise ValueError(f"state must hold {state_size(classes)} integers for {classes} classes, got {s.dtype} x {s.size}")
    s = s.astype(np.int64).reshape(-1)
    cc = classes * classes
    cm = s[:cc].reshape(classes, classes).copy()
    thick = s[cc:cc + classes]
    columns, ignored, invalid, updates = (int(v) for v in s[cc + classes:])
    n = int(cm.sum())
    t, p, tp = cm.sum(axis=1), cm.sum(axis=0), np.diagonal(cm)
    counts = np.stack([tp, t, p, n - t - p + tp, p - tp, t - tp], axis=1).astype(np.int64)
    per = [_formulas(*(int(v) for v in row), n) for row in counts]
    res = {k: np.array([d[k] for d in per], dtype=np.float64) for k in per[0]}
    present = (t + p) > 0
    res.update({
        "confusion": cm, "counts": counts, "present": present,
        "pixel_accuracy": float(tp.sum()) / n if n else float("nan"),
        "mean_dice": float(res["dice_coefficient"][present].mean()) if present.any() else float("nan"),
        "mean_iou": float(res["iou_score"][present].mean()) if present.any() else float("nan"),
        "thickness_error": thick.astype(np.float64) / columns if columns else np.full(classes, np.nan),
        "n": n, "ignored": ignored, "invalid": invalid, "columns": columns, "updates": updates,
    })
    return res


def _class_map(t, what):
    """an integer class map (..., H, W) as the kernel reads it: uint8 or int64, contiguous"""
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a torch tensor, got {type(t).__name__}")
    if t.dtype not in _INT_DTYPES:
        raise TypeError(f"{what} must be an integer class map, got {t.dtype}")
    if t.dim() < 2:
        raise RuntimeError(f"{what} must have shape (..., H, W), got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype not in (torch.uint8, torch.int64):
        t = t.to(torch.int64)
    return t.contiguous()


class SegEvaluator:
    """Confusion matrix + per-layer thickness error of a validation set, accumulated on the device."""

    def __init__(self, classes, ignore_index=None, device=None):
        _check_config(classes, ignore_index)
        self.classes = classes
        self.ignore_index = ignore_index
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type != "cuda":
            raise L.OctError("SegEvaluator needs a GPU device: there is no CPU fallback on the product path")
        self.state = None   # int64 [C*C + C + 4] on the device, allocated by the first update

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _state_on(self, device):
        if device.type != "cuda":
            raise L.OctError("the HIP path needs a device tensor (there is no CPU fallback)")
        if self.state is None:
            if self.device is not None and self.device.index is not None and device != self.device:
                raise RuntimeError(f"inputs are on {device}, the evaluator was made for {self.device}")
            self.state = torch.zeros(state_size(self.classes), dtype=torch.int64, device=device)
        elif self.state.device != device:
            raise RuntimeError(f"inputs are on {device}, the evaluator's state on {self.state.device}")
        return self.state

    def reset(self):
        if self.state is not None:
            self.state.zero_()
        return self

    def _launch(self, target, pred, kind, images, h, w):
        if images * h * w >= 2 ** 31:
            raise RuntimeError(f"one update takes fewer than 2^31 pixels, got {images} x {h} x {w}")
        state = self._state_on(target.device)
        desc = L.SegEvalDesc(images, h, w, self.classes, 0 if target.dtype == torch.uint8 else 2, kind,
                             int(self.ignore_index is not None), int(self.ignore_index or 0))
        L.check(L.lib().oct_seg_eval_update(C.byref(desc), target.data_ptr(), pred.data_ptr(), state.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "oct_seg_eval_update")
        return self

    # ---- updates ----------------------------------------------------------------------------------------------------------
    def update(self, target, pred):
        """Two integer class maps of one shape (..., H, W): uint8 and int64 are read as they are (each side its own type),
        other integer dtypes are converted to int64.  Every leading dimension counts images."""
        target, pred = _class_map(target, "target"), _class_map(pred, "pred")
        if target.shape != pred.shape:
            raise RuntimeError(f"target {tuple(target.shape)} and pred {tuple(pred.shape)} must have the same shape")
        if target.device != pred.device:
            raise RuntimeError(f"target is on {target.device}, pred on {pred.device}")
        h, w = target.shape[-2:]
        if h < 1 or w < 1:
            raise RuntimeError(f"class maps need H, W >= 1, got {tuple(target.shape)}")
        images = target.numel() // (h * w)
        kind = L.EVAL_PRED_U8 if pred.dtype == torch.uint8 else L.EVAL_PRED_I64
        return self._launch(target, pred, kind, images, h, w)

    def update_logits(self, target, logits, layout="nhwc"):
        """target (N, H, W) against the arg-max of logits -- NHWC bf16 / fp32 (what the logits networks write) or NCHW fp32
        (what a forward returns) -- taken inside the kernel with model.predict's rule (first maximum wins): no class map
        is written."""
        if layout not in _LAYOUTS:
            raise ValueError(f"layout must be 'nhwc' or 'nchw', got {layout!r}")
        lay = _LAYOUTS[layout]
        if not torch.is_tensor(logits) or logits.dim() != 4:
            raise RuntimeError(f"expected 4-D logits, got {tuple(logits.shape) if torch.is_tensor(logits) else type(logits).__name__}")
        if lay == L.SEG_NCHW:
            if logits.dtype != torch.float32:
                raise L.OctError(f"NCHW logits must be fp32 (got {logits.dtype})")
            n, c, h, w = logits.shape
            kind = L.EVAL_PRED_NCHW_F32
        else:
            if logits.dtype not in (torch.bfloat16, torch.float32):
                raise L.OctError(f"NHWC logits must be bf16 or fp32 (got {logits.dtype})")
            n, h, w, c = logits.shape
            kind = L.EVAL_PRED_NHWC_BF16 if logits.dtype == torch.bfloat16 else L.EVAL_PRED_NHWC_F32
        if c != self.classes:
            raise RuntimeError(f"the logits have {c} channels, the evaluator {self.classes} classes")
        target = _class_map(target, "target")
        if tuple(target.shape) != (n, h, w):
            raise RuntimeError(f"target must have shape {(n, h, w)}, got {tuple(target.shape)}")
        if target.device != logits.device:
            raise RuntimeError(f"target is on {target.device}, logits on {logits.device}")
        if h < 1 or w < 1:
            raise RuntimeError(f"logits need H, W >= 1, got {tuple(logits.shape)}")
        return self._launch(target, logits.detach().contiguous(), kind, n, h, w)

    @torch.no_grad()
    def update_model(self, model, x, target):
        """Forward of `model` in its current mode, then one update: the engine networks (UNet, BioUNet, UNet3D) through
        model.predict(x) -- a UNet3D map (B, D, H, W) counts B*D images -- the logits networks (SegLossMixin) straight from
        their NHWC logits."""
        from .losses import SegLossMixin
        from .unet import _EngineNet
        if isinstance(model, SegLossMixin):
            ncls, logits_net = model._classes(), True
        elif isinstance(model, _EngineNet):
            ncls, logits_net = model._engine.ncls, False
        else:
            raise TypeError(f"update_model takes one of this package's networks, got {type(model).__name__}")
        if ncls != self.classes:
            raise RuntimeError(f"{type(model).__name__} has {ncls} classes, the evaluator {self.classes}")
        if not torch.is_tensor(x) or x.dim() < 4:
            raise RuntimeError(f"expected a batched input (B, C, ..., H, W), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        want = (x.shape[0],) + tuple(x.shape[2:])
        if not torch.is_tensor(target) or tuple(target.shape) != want:
            raise RuntimeError(f"target must have shape {want}, got {tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
        if target.device != x.device:
            raise RuntimeError(f"target is on {target.device}, the input on {x.device}")
        _class_map(target, "target")
        if logits_net:
            return self.update_logits(target, model._run_logits(x), "nhwc")
        return self.update(target, model.predict(x))

    # ---- results ----------------------------------------------------------------------------------------------------------
    def all_reduce(self, group=None):
        """Sum the state over the ranks of `group` (one all-reduce of C*C + C + 4 int64); nothing to do in one process."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if self.state is None:   # a rank without a batch still takes part
            self._state_on(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    def compute(self) -> dict:
        """The only call that synchronises: reads the state and returns
          confusion [C, C] int64; counts [C, 6] int64 = tp, t, p, tn, fp, fn one-vs-rest with n = valid pixels;
          every key of Metrics._formulas as a float64 array over the classes; pixel_accuracy; present = t + p > 0;
          mean_dice / mean_iou over the present classes; thickness_error = thick_abs / columns in pixels (NaN without a
          column); n, ignored, invalid, columns, updates."""
        if self.state is None:
            return metrics_from_state(np.zeros(state_size(self.classes), dtype=np.int64), self.classes)
        return metrics_from_state(self.state.cpu().numpy(), self.classes)
