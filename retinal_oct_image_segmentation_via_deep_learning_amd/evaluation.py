"""Streaming validation metrics with the state on the device.

A validation loop scores batch after batch; `Metrics.evaluate(y_true, y_pred, classes=C)` reads its counts back per batch and
knows neither a C x C confusion matrix nor ignore_index.  The evaluators here keep their result on the device: update()
launches on the stream of its tensors' device and never synchronises, compute() is the only call that reads back, and there
is no CPU fallback.  What they share is written once: `_Evaluator` (the device= argument and the three device rules of
_bind), `_StateEvaluator` (one summable int64 state: state, reset, all_reduce, _host_state -- SegEvaluator, ScoreEvaluator,
LesionEvaluator, SurfaceEvaluator; BoundaryEvaluator's records are per image and not summable) and the plain functions below
it for class-map pairs, image chunks under a workspace limit, the cached workspace and the model dispatch of update_model.

Confusion matrix and thickness (csrc/seg_eval.hip, oct_seg_eval_update): `SegEvaluator` ADDS to one int64 buffer per update

    cm[t*C + p] | thick_abs[c] | columns | ignored | invalid | updates            (C*C + C + 4 entries)

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

Contour metrics (csrc/contour.hip, oct_contour_update): `BoundaryEvaluator` keeps, per image, class and direction, five exact
int64 values on the device -- Hausdorff, HD95 and ASSD follow from them in `contour_metrics_from_records` (numpy, float64).

  contour points of a mask M   the midpoints of the in-image pairs of 4-adjacent pixels with exactly one pixel in M: the vertex
                               set of marching squares at level 0.5 (skimage.find_contours(M, 0.5)).  None along the image
                               border: a full or an empty mask has no contour.  In doubled coordinates (2y, 2x+1) / (2y+1, 2x)
                               the points are integral; D2 = squared distance there, true distance sqrt(D2) / 2 pixels.
  classes                      M_c = {label == c}; a pixel whose target equals ignore_index is outside the image in both maps;
                               labels outside [0, C) belong to no class.
  record [image, c, dir]       n, max_d2, lo_d2, hi_d2, sum_q.  dir 0: from the points of pred to the nearest point of target
                               (the reference's d1), dir 1 the reverse.  lo = 19 (n - 1) // 20, hi = min(lo + 1, n - 1) are the
                               ranks np.percentile(., 95) interpolates between; sum_q = sum floor(2^16 sqrt(D2)).
  f(v) = sqrt(v) / 2           HD = max_dir f(max_d2);  HD95 = max_dir f(lo) + frac (f(hi) - f(lo)), frac = (19 (n-1) % 20) / 20;
                               ASSD = (sum_q[0] / n[0] + sum_q[1] / n[1]) / 2 / 2^17 (truncation <= 2^-17 px).  NaN unless
                               both sides have a point.

Score evaluator (csrc/score_eval.hip, oct_score_eval_update): `ScoreEvaluator` validates a binary / multi-label (sigmoid) head
without a threshold -- per channel one [2][65536] histogram of a 16-bit order-preserving key of the score by label, in one
int64 device buffer; ROC AUC, average precision, the confusion counts at any threshold chosen afterwards and the best-Dice
threshold follow from it in `score_metrics_from_state` (numpy, exact integers).  The key: `key16`.

Lesion-wise scores (csrc/components.hip, oct_lesion_eval_update): `LesionEvaluator` labels both maps into connected components
(same value, 4- or 8-neighbours; postprocess.py has the labelling itself and the cleanup filter) and keeps, per class, four
int64 counts on the device -- target components, predicted components, detected, confirmed; sensitivity, precision and F1 per
lesion follow from them in `lesion_metrics_from_state` (numpy, float64).

Surface position error (csrc/surfaces.hip, oct_surf_error_update): `SurfaceEvaluator` compares two sets of layer surfaces
(surfaces.py: one boundary row per A-scan and interface) and keeps, per surface, five int64 values on the device -- columns,
sum |e|, sum e, sum e^2, max |e|; mean absolute, signed and RMS error in pixels follow in `surface_metrics_from_state`.

Deviations from the reference's Metrics/Contour_based_metrics.py, by decision: it scores only the FIRST contour find_contours
returns (order-dependent) and counts the first vertex of a closed contour twice; here every contour counts and every vertex
once.  For one simply connected object off the border hausdorff_distance is the same value, HD95 and ASSD differ by the weight
of the repeated vertex.  Where the reference raises IndexError (a mask without a contour) the result is NaN.  skimage is not a
dependency, so parity with the reference is by construction and not pinned by a test.
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


def _check_int(name, value, lo, hi, none_ok=False, out_of_range=None):
    """value is an int (not a bool) in [lo, hi], or None where none_ok; out_of_range replaces the range message"""
    if value is None and none_ok:
        return
    if isinstance(value, bool) or not isinstance(value, int):
        raise TypeError(f"{name} must be an int{' or None' if none_ok else ''}, got {type(value).__name__} {value!r}")
    if not lo <= value <= hi:
        raise ValueError(out_of_range or f"{name} must be in {lo}..{hi} (got {value})")


def _check_config(classes, ignore_index):
    _check_int("classes", classes, 1, L.MAX_CLASSES)
    _check_int("ignore_index", ignore_index, -2 ** 63, 2 ** 63 - 1, True, f"ignore_index {ignore_index} is not an int64")


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")


def _check_workspace_limit(max_workspace_bytes):
    if isinstance(max_workspace_bytes, bool) or not isinstance(max_workspace_bytes, int) or max_workspace_bytes < 1:
        raise ValueError(f"max_workspace_bytes must be a positive int, got {max_workspace_bytes!r}")


def _int_state(state, size, what):
    """an evaluator's state as a flat int64 array of exactly `size` entries; `what` names the configuration in the message"""
    s = np.asarray(state)
    if s.dtype.kind not in "iu" or s.size != size:
        raise ValueError(f"state must hold {size} integers for {what}, got {s.dtype} x {s.size}")
    return s.astype(np.int64).reshape(-1)


def metrics_from_state(state, classes: int) -> dict:
    """Every metric of the evaluator from its int64 state (numpy, no GPU): see SegEvaluator.compute."""
    from .Metrics import _formulas
    _check_config(classes, None)
    s = _int_state(state, state_size(classes), f"{classes} classes")
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


def _elem(t):
    """the kernels' element code of a class map: uint8 (0) or int64 (2)"""
    return 0 if t.dtype == torch.uint8 else 2


def _map_geometry(m, max_dim=None, limit_what=None):
    """(images, h, w) of a class map (..., H, W): H, W >= 1 and, with max_dim, at most that"""
    h, w = m.shape[-2:]
    if h < 1 or w < 1:
        raise RuntimeError(f"class maps need H, W >= 1, got {tuple(m.shape)}")
    if max_dim is not None and (h > max_dim or w > max_dim):
        raise RuntimeError(f"{limit_what} take H, W <= {max_dim}, got {h} x {w}")
    return m.numel() // (h * w), h, w


def _class_map_pair(target, pred, max_dim=None, limit_what=None):
    """Two integer class maps of one shape on one device as the kernels read them, and (images, h, w).  No device rule is
    applied here: that is the evaluator's _bind, after every check that needs no device."""
    target, pred = _class_map(target, "target"), _class_map(pred, "pred")
    if target.shape != pred.shape:
        raise RuntimeError(f"target {tuple(target.shape)} and pred {tuple(pred.shape)} must have the same shape")
    if target.device != pred.device:
        raise RuntimeError(f"target is on {target.device}, pred on {pred.device}")
    return target, pred, _map_geometry(target, max_dim, limit_what)


def _image_chunks(images, h, w, one, max_workspace_bytes):
    """(lo, k) over images >= 1 in order: k images from lo on, the largest k whose workspace fits max_workspace_bytes given
    that one image takes `one` bytes (bytes(k) <= k * bytes(1)) and whose k * h * w stays below 2^31.  An image that does not
    fit raises here, before the first chunk is asked for."""
    if one > max_workspace_bytes:
        raise RuntimeError(f"one {h} x {w} image needs a workspace of {one} bytes, max_workspace_bytes is {max_workspace_bytes}")
    per = min(images, max_workspace_bytes // one, max(1, (2 ** 31 - 1) // (h * w)))
    return ((lo, min(per, images - lo)) for lo in range(0, images, per))


def _grown(buf, need, device):
    """the cached uint8 workspace `buf`, or a new one where it is missing, too small or on another device"""
    if buf is None or buf.numel() < need or buf.device != device:
        return torch.empty(need, dtype=torch.uint8, device=device)
    return buf


def _model_kind(model):
    """(classes, hands_out_logits) of one of this package's networks: the logits networks (SegLossMixin) write NHWC logits,
    the engine networks (UNet, BioUNet, UNet3D) answer through predict() / logits()"""
    from .losses import SegLossMixin
    from .unet import _EngineNet
    if isinstance(model, SegLossMixin):
        return model._classes(), True
    if isinstance(model, _EngineNet):
        return model._engine.ncls, False
    raise TypeError(f"update_model takes one of this package's networks, got {type(model).__name__}")


class _Evaluator:
    """What every evaluator shares: the device= argument and the device rules of its inputs."""

    def __init__(self, device):
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type != "cuda":
            raise L.OctError(f"{type(self).__name__} needs a GPU device: there is no CPU fallback on the product path")

    def _bind(self, device, held, what):
        """`device` (that of the inputs) is a GPU, the one the evaluator was made for, and the one of the tensor it already
        holds (`held`, named `what` in the message; None before the first update)"""
        if device.type != "cuda":
            raise L.OctError("the HIP path needs a device tensor (there is no CPU fallback)")
        if self.device is not None and self.device.index is not None and device != self.device:
            raise RuntimeError(f"inputs are on {device}, the evaluator was made for {self.device}")
        if held is not None and held.device != device:
            raise RuntimeError(f"inputs are on {device}, the evaluator's {what} on {held.device}")


class _StateEvaluator(_Evaluator):
    """An evaluator whose result is one int64 device buffer of `size` entries that every update ADDS to, so that the states
    of several ranks sum."""

    def __init__(self, device, size):
        super().__init__(device)
        self._size = size
        self.state = None   # int64 [size] on the device, allocated by the first update

    def _state_on(self, device):
        self._bind(device, self.state, "state")
        if self.state is None:
            self.state = torch.zeros(self._size, dtype=torch.int64, device=device)
        return self.state

    def reset(self):
        if self.state is not None:
            self.state.zero_()
        return self

    def all_reduce(self, group=None):
        """Sum the state over the ranks of `group` (one SUM all-reduce of the int64 state); nothing to do in one process."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if self.state is None:   # a rank without a batch still takes part
            self._state_on(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    def _host_state(self):
        """the state as a numpy array (zeros before the first update): the one synchronisation"""
        if self.state is None:
            return np.zeros(self._size, dtype=np.int64)
        return self.state.cpu().numpy()


class SegEvaluator(_StateEvaluator):
    """Confusion matrix + per-layer thickness error of a validation set, accumulated on the device."""

    def __init__(self, classes, ignore_index=None, device=None):
        _check_config(classes, ignore_index)
        super().__init__(device, state_size(classes))
        self.classes = classes
        self.ignore_index = ignore_index

    def _launch(self, target, pred, kind, images, h, w):
        if images * h * w >= 2 ** 31:
            raise RuntimeError(f"one update takes fewer than 2^31 pixels, got {images} x {h} x {w}")
        state = self._state_on(target.device)
        desc = L.SegEvalDesc(images, h, w, self.classes, _elem(target), kind,
                             int(self.ignore_index is not None), int(self.ignore_index or 0))
        L.check(L.lib().oct_seg_eval_update(C.byref(desc), target.data_ptr(), pred.data_ptr(), state.data_ptr(),
                                            torch.cuda.current_stream(target.device).cuda_stream), "oct_seg_eval_update")
        return self

    # ---- updates ----------------------------------------------------------------------------------------------------------
    def update(self, target, pred):
        """Two integer class maps of one shape (..., H, W): uint8 and int64 are read as they are (each side its own type),
        other integer dtypes are converted to int64.  Every leading dimension counts images."""
        target, pred, (images, h, w) = _class_map_pair(target, pred)
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
        ncls, logits_net = _model_kind(model)
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

    def compute(self) -> dict:
        """The only call that synchronises: reads the state and returns
          confusion [C, C] int64; counts [C, 6] int64 = tp, t, p, tn, fp, fn one-vs-rest with n = valid pixels;
          every key of Metrics._formulas as a float64 array over the classes; pixel_accuracy; present = t + p > 0;
          mean_dice / mean_iou over the present classes; thickness_error = thick_abs / columns in pixels (NaN without a
          column); n, ignored, invalid, columns, updates."""
        return metrics_from_state(self._host_state(), self.classes)


# ---- contour metrics ------------------------------------------------------------------------------------------------------
RECORD_FIELDS = ("n", "max_d2", "lo_d2", "hi_d2", "sum_q")


def contour_metrics_from_records(records) -> dict:
    """Hausdorff, HD95 and ASSD from the int64 records [images, C, 2, 5] (numpy float64, no GPU): see
    BoundaryEvaluator.compute and the formulas in the module doc-string."""
    r = np.asarray(records)
    if r.dtype.kind not in "iu" or r.ndim != 4 or r.shape[2:] != (2, len(RECORD_FIELDS)):
        raise ValueError(f"records must be integers of shape [images, C, 2, 5], got {r.dtype} {r.shape}")
    r = r.astype(np.int64)
    n, max_d2, lo_d2, hi_d2, sum_q = (r[..., k] for k in range(5))          # each [images, C, 2]
    defined = (n > 0).all(axis=2)

    def f(v):
        return np.sqrt(v.astype(np.float64)) / 2.0

    frac = ((19 * (n - 1)) % 20).astype(np.float64) / 20.0
    flo = f(lo_d2)
    p95 = flo + frac * (f(hi_d2) - flo)
    mean_q = sum_q.astype(np.float64) / np.where(n > 0, n, 1)
    nan = np.float64("nan")
    res = {
        "hausdorff": np.where(defined, f(max_d2).max(axis=2), nan),
        "hd95": np.where(defined, p95.max(axis=2), nan),
        "assd": np.where(defined, (mean_q[..., 0] + mean_q[..., 1]) / 2.0 / 2.0 ** 17, nan),
        "defined": defined,
        "images": int(r.shape[0]),
    }
    count = defined.sum(axis=0)
    for k in ("hausdorff", "hd95", "assd"):
        total = np.where(defined, res[k], 0.0).sum(axis=0)
        res["mean_" + k] = np.where(count > 0, total / np.where(count > 0, count, 1), nan)
    return res


class BoundaryEvaluator(_Evaluator):
    """Hausdorff / HD95 / ASSD per image and class of a validation set; the records stay on the device until compute()."""

    def __init__(self, classes, ignore_index=None, device=None, max_workspace_bytes=256 << 20):
        _check_config(classes, ignore_index)
        _check_workspace_limit(max_workspace_bytes)
        super().__init__(device)
        self.classes = classes
        self.ignore_index = ignore_index
        self.max_workspace_bytes = max_workspace_bytes
        self._chunks = []        # int64 [images_i, C, 2, 5] device tensors, in update order
        self._workspace = None   # uint8 device buffer, grown on demand, reused by every update

    def _desc(self, images, h, w, target, pred):
        return L.ContourDesc(images, h, w, self.classes, _elem(target), _elem(pred), int(self.ignore_index is not None),
                             int(self.ignore_index or 0))

    def reset(self):
        self._chunks = []
        return self

    def update(self, target, pred):
        """Two integer class maps of one shape (..., H, W), H, W <= 16384, with SegEvaluator.update's input rules.  The batch
        goes through the kernel in chunks of images whose workspace fits max_workspace_bytes; one image that does not fit
        raises.  Nothing is read back."""
        target, pred, (images, h, w) = _class_map_pair(target, pred, L.CONTOUR_MAX_DIM, "contour metrics")
        self._bind(target.device, self._chunks[0] if self._chunks else None, "records")
        if images == 0:
            return self
        lib = L.lib()
        one = int(lib.oct_contour_workspace_bytes(C.byref(self._desc(1, h, w, target, pred))))
        if one == 0:
            raise L.OctError(f"oct_contour_workspace_bytes failed: {L.last_error()}")
        chunks = _image_chunks(images, h, w, one, self.max_workspace_bytes)
        target, pred = target.reshape(images, h, w), pred.reshape(images, h, w)
        out = torch.empty((images, self.classes, 2, len(RECORD_FIELDS)), dtype=torch.int64, device=target.device)
        stream = torch.cuda.current_stream(target.device).cuda_stream
        for lo, k in chunks:
            desc = self._desc(k, h, w, target, pred)
            need = int(lib.oct_contour_workspace_bytes(C.byref(desc)))
            self._workspace = _grown(self._workspace, need, target.device)
            L.check(lib.oct_contour_update(C.byref(desc), target[lo:lo + k].data_ptr(), pred[lo:lo + k].data_ptr(),
                                           out[lo:lo + k].data_ptr(), self._workspace.data_ptr(), stream), "oct_contour_update")
        self._chunks.append(out)
        return self

    @torch.no_grad()
    def update_model(self, model, x, target):
        """model.predict(x) of an engine network (UNet, BioUNet, UNet3D) against target; the logits networks have no class
        map of their own: pass theirs to update(target, class_map)."""
        ncls, logits_net = _model_kind(model)
        if logits_net:
            raise TypeError(f"update_model takes an engine network with predict(); for {type(model).__name__} call "
                            "update(target, class_map) with its arg-max")
        if ncls != self.classes:
            raise RuntimeError(f"{type(model).__name__} has {ncls} classes, the evaluator {self.classes}")
        return self.update(target, model.predict(x))

    def merge(self, records):
        """Append records gathered elsewhere (another rank's records(), as a tensor or an array [images, C, 2, 5])."""
        if not torch.is_tensor(records):
            records = torch.from_numpy(np.ascontiguousarray(np.asarray(records)))
        if records.dtype != torch.int64 or records.dim() != 4 or tuple(records.shape[1:]) != (self.classes, 2, len(RECORD_FIELDS)):
            raise ValueError(f"records must be int64 [images, {self.classes}, 2, 5], got {records.dtype} {tuple(records.shape)}")
        if self._chunks:
            records = records.to(self._chunks[0].device)
        self._chunks.append(records)
        return self

    def records(self):
        """int64 [images, C, 2, 5] on the device, in update order (an empty CPU tensor before the first update)."""
        if not self._chunks:
            return torch.zeros((0, self.classes, 2, len(RECORD_FIELDS)), dtype=torch.int64)
        if len(self._chunks) > 1:
            self._chunks = [torch.cat(self._chunks, dim=0)]
        return self._chunks[0]

    def compute(self) -> dict:
        """The only call that synchronises: per-image float64 arrays hausdorff, hd95, assd [images, C] in pixels (NaN where
        a side has no contour), defined [images, C] bool, mean_hausdorff / mean_hd95 / mean_assd [C] over the defined images
        (NaN without one), images."""
        return contour_metrics_from_records(self.records().cpu().numpy())


# ---- score evaluator: ROC AUC, average precision and threshold sweeps per channel -------------------------------------------
SCORE_KEYS = L.SCORE_KEYS
_SCORE_ELEM = {torch.float32: L.SCORE_F32, torch.bfloat16: L.SCORE_BF16, torch.uint8: L.SCORE_U8}


def score_state_size(channels: int) -> int:
    return channels * (2 * SCORE_KEYS + 3) + 1


def key16(v):
    """The 16-bit key of float32 scores (numpy, any shape; the values must not be NaN): the order-preserving code of v rounded
    toward -inf onto the bf16 grid.  With u = bits(v), h = u >> 16, low = u & 0xFFFF:
      sign clear:  key = 0x8000 + h
      sign set:    m = (h & 0x7FFF) + (low != 0), capped at 0x7F80;  key = 0x8000 - m
    -0.0 and +0.0 share key 0x8000; keys lie in [0x0080, 0xFF80]; bin k is the half-open interval [g(k), g(k+1)) of the real
    line, g = key_value.  For a threshold theta on the bf16 grid v >= theta <=> key16(v) >= key16(theta) for every fp32 v,
    negative theta included (hence rounding toward -inf, not truncation); theta = 0 is on the grid."""
    a = np.asarray(v, dtype=np.float32)
    u = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.int64).reshape(a.shape)
    h, low = u >> 16, u & 0xFFFF
    m = np.minimum((h & 0x7FFF) + (low != 0), 0x7F80)
    return np.where(u >> 31 != 0, 0x8000 - m, 0x8000 + h)


def key_value(k):
    """g(k): the lower edge of bin k as float32 (the bf16 value whose key is k)"""
    k = np.asarray(k, dtype=np.int64)
    bits = np.where(k >= 0x8000, (k - 0x8000) << 16, 0x80000000 | ((0x8000 - k) << 16))
    return bits.astype(np.uint32).view(np.float32)


def _check_score_config(channels, ignore_value):
    _check_int("channels", channels, 1, L.MAX_CLASSES)
    _check_int("ignore_value", ignore_value, 2, 255, True,
               f"ignore_value {ignore_value} is not in [2, 255] (0 and 1 are the mask's own values)")


def _score_hist(state, channels):
    _check_score_config(channels, None)
    s = _int_state(state, score_state_size(channels), f"{channels} channels")
    nh = channels * 2 * SCORE_KEYS
    return s[:nh].reshape(channels, 2, SCORE_KEYS), s[nh:]


def _threshold_keys(thresholds, logits):
    from .losses import mask_threshold
    theta = [mask_threshold(t) if logits else t for t in thresholds]
    theta = np.array(theta, dtype=np.float32).reshape(-1)
    if np.isnan(theta).any():
        raise ValueError(f"thresholds must not be NaN, got {thresholds!r}")
    return key16(theta)


def _occupied(hist_c):
    """occupied keys (ascending) of one channel with their counts as Python ints"""
    neg, pos = hist_c[0], hist_c[1]
    keys = np.flatnonzero((neg != 0) | (pos != 0))
    return keys, [int(v) for v in neg[keys]], [int(v) for v in pos[keys]]


def _pair_counts(neg, pos):
    """P, N, sum_k pos_k neg_below_k and sum_k pos_k neg_k over the occupied keys in ascending order, as exact Python ints"""
    below = wins = ties = 0
    for n, p in zip(neg, pos):
        wins += p * below
        ties += p * n
        below += n
    return sum(pos), below, wins, ties


def _auc_from_state(state):
    """(auc | None, nan, invalid) of a one-channel state: the AUC alone, for Metrics.auc_score"""
    hist, tail = _score_hist(state, 1)
    _, neg, pos = _occupied(hist[0])
    P, N, wins, ties = _pair_counts(neg, pos)
    return ((2 * wins + ties) / (2 * P * N) if P and N else None), int(tail[0]), int(tail[2])


def score_curves_from_state(state, channels: int, channel: int) -> dict:
    """ROC and precision-recall points of one channel over its occupied keys in DESCENDING order (numpy, no GPU):
    thresholds = key_value(key) float32, tp / fp = the counts of key >= that key (int64), tpr = tp / P, fpr = fp / N,
    precision = tp / (tp + fp), recall = tpr.  NaN where a label is missing."""
    hist, _ = _score_hist(state, channels)
    if not 0 <= channel < channels:
        raise ValueError(f"channel must be in 0..{channels - 1}, got {channel}")
    keys, neg, pos = _occupied(hist[channel])
    keys, neg, pos = keys[::-1], neg[::-1], pos[::-1]
    tp, fp, a, b = [], [], 0, 0
    for n, p in zip(neg, pos):
        a, b = a + p, b + n
        tp.append(a)
        fp.append(b)
    nan = float("nan")
    return {
        "thresholds": key_value(keys),
        "tp": np.array(tp, dtype=np.int64), "fp": np.array(fp, dtype=np.int64),
        "tpr": np.array([t / a if a else nan for t in tp], dtype=np.float64),
        "fpr": np.array([f / b if b else nan for f in fp], dtype=np.float64),
        "precision": np.array([t / (t + f) for t, f in zip(tp, fp)], dtype=np.float64),
    }


def score_metrics_from_state(state, channels: int, thresholds=(0.5,), logits=True) -> dict:
    """Every figure of the score evaluator from its int64 state (numpy, no GPU), per channel.

    With 16-bit scores (bf16 logits or probabilities, uint8 images) everything is exact.  With fp32 scores the counts at a
    threshold theta are those at threshold_used <= theta (the lower edge of theta's bin; equal when theta is on the bf16 grid,
    as 0 is), and the AUC is bracketed by [auc_lo, auc_hi], not exact: `auc` counts every pair inside one bin as a tie.

      positives, negatives, nan, ignored, invalid   int64 [C];  updates int
      auc                 (sum_k pos_k neg_below_k + 1/2 sum_k pos_k neg_k) / (P N): ties count half, sklearn's trapezoid.
                          NaN unless both labels are present
      auc_lo, auc_hi      the same with the tie term counted 0 and 1;  hi - lo = sum_k pos_k neg_k / (P N)
      average_precision   sum_i (R_i - R_{i-1}) P_i over the occupied keys in descending order (sklearn); NaN without a positive
      threshold_used [T]  float32 key_value(key16(theta)), theta = losses.mask_threshold(tau) with logits, float32(tau) without
      counts [C, T, 6]    int64 tp, t, p, tn, fp, fn of key >= key16(theta), the argument order of Metrics._formulas;
                          every key of Metrics._formulas as a float64 [C, T] array
      best_dice, best_dice_threshold   the maximum of _formulas' Dice over all occupied keys as thresholds, and the largest
                          threshold (float32) that attains it; NaN without an occupied key
    Products of counts are exact Python integers (P N passes 2^63 on a real validation set); one float64 division ends each."""
    import math
    from .Metrics import _formulas
    hist, tail = _score_hist(state, channels)
    tkeys = _threshold_keys(thresholds, logits)
    nt, nan = len(tkeys), float("nan")
    res = {"nan": tail[:channels].copy(), "ignored": tail[channels:2 * channels].copy(),
           "invalid": tail[2 * channels:3 * channels].copy(), "updates": int(tail[3 * channels]),
           "positives": hist[:, 1].sum(axis=1), "negatives": hist[:, 0].sum(axis=1),
           "threshold_used": key_value(tkeys)}
    auc, lo, hi, ap = (np.full(channels, nan) for _ in range(4))
    best, best_thr = np.full(channels, nan), np.full(channels, nan, dtype=np.float32)
    counts = np.zeros((channels, nt, 6), dtype=np.int64)
    for c in range(channels):
        keys, neg, pos = _occupied(hist[c])
        P, N, wins, ties = _pair_counts(neg, pos)
        if P and N:
            auc[c], lo[c], hi[c] = (2 * wins + ties) / (2 * P * N), wins / (P * N), (wins + ties) / (P * N)
        # descending sweep: average precision and the best Dice
        tp = fp = 0
        terms = []
        for k, n, p in zip(keys[::-1], neg[::-1], pos[::-1]):
            tp, fp = tp + p, fp + n
            terms.append((p * tp) / (tp + fp))
            d = _formulas(tp, P, tp + fp, N - fp, fp, P - tp, P + N)["dice_coefficient"]
            if not best[c] >= d:   # strictly better, or the first: ties keep the larger threshold
                best[c], best_thr[c] = d, key_value(k)
        if P:
            ap[c] = math.fsum(terms) / P
        above_pos = np.concatenate([np.cumsum(hist[c, 1][::-1])[::-1], [0]])
        above_neg = np.concatenate([np.cumsum(hist[c, 0][::-1])[::-1], [0]])
        for i, k in enumerate(tkeys):
            tp, fp = int(above_pos[k]), int(above_neg[k])
            counts[c, i] = (tp, P, tp + fp, N - fp, fp, P - tp)
    res.update({"auc": auc, "auc_lo": lo, "auc_hi": hi, "average_precision": ap, "counts": counts,
                "best_dice": best, "best_dice_threshold": best_thr})
    n_all = res["positives"] + res["negatives"]
    per = [[_formulas(*(int(v) for v in counts[c, i]), int(n_all[c])) for i in range(nt)] for c in range(channels)]
    for k in _formulas(0, 0, 0, 0, 0, 0, 0):
        res[k] = np.array([[per[c][i][k] for i in range(nt)] for c in range(channels)], dtype=np.float64).reshape(channels, nt)
    return res


class ScoreEvaluator(_StateEvaluator):
    """Threshold-free validation of a binary / multi-label head, accumulated on the device (csrc/score_eval.hip): per channel
    ONE [2][65536] histogram of key16(score) by label in the int64 state

        hist[C][2][65536] | nan[C] | ignored[C] | invalid[C] | updates

    Each element goes to one place: ignored (ignore_value given and t == ignore_value), else invalid (t > 1), else nan (the
    score is NaN), else hist[c][t][key16(score)].

        ev = ScoreEvaluator(channels=3, ignore_value=255, logits=True)
        for x, y in loader:
            ev.update_model(model, x, y)        # or ev.update(y, scores, layout="nchw" | "nhwc")
        ev.all_reduce()
        m = ev.compute(thresholds=(0.5, 0.3))   # auc, average_precision, counts at any threshold, best_dice, ...

    `logits` only decides how compute(thresholds=...) maps a probability threshold tau into score space: True through
    losses.mask_threshold(tau) (predict_mask's rule), False as float32(tau).  What is exact and what is bracketed:
    score_metrics_from_state."""

    def __init__(self, channels, ignore_value=None, logits=True, device=None):
        _check_score_config(channels, ignore_value)
        super().__init__(device, score_state_size(channels))
        self.channels = channels
        self.ignore_value = ignore_value
        self.logits = bool(logits)

    def _launch(self, target, scores, images, h, w):
        """target uint8 and scores, both contiguous [images][channels][h][w] on one device"""
        state = self._state_on(target.device)
        desc = L.ScoreEvalDesc(images, h, w, self.channels, _SCORE_ELEM[scores.dtype], int(self.ignore_value is not None),
                               int(self.ignore_value or 0))
        L.check(L.lib().oct_score_eval_update(C.byref(desc), target.data_ptr(), scores.data_ptr(), state.data_ptr(),
                                              torch.cuda.current_stream(target.device).cuda_stream), "oct_score_eval_update")
        return self

    def update(self, target, scores, layout="nchw"):
        """scores (B, C, H, W) fp32 / bf16 / uint8 ("nchw"; (B, H, W) is accepted for one channel) or (B, H, W, C) fp32 / bf16
        ("nhwc": the logits networks' own output, taken through oct_nhwc_to_nchw to planar fp32 first -- an exact conversion,
        so both layouts of the same values give the same state).  target: uint8 / bool (B, C, H, W), or (B, H, W) for one
        channel (losses._binary_target's rules).  fp16 is refused: its mantissa does not fit the key."""
        from .losses import _binary_target
        if layout not in _LAYOUTS:
            raise ValueError(f"layout must be 'nhwc' or 'nchw', got {layout!r}")
        lay = _LAYOUTS[layout]
        if not torch.is_tensor(scores):
            raise TypeError(f"scores must be a torch tensor, got {type(scores).__name__}")
        if scores.dtype == torch.bool:
            scores = scores.view(torch.uint8)
        if lay == L.SEG_NCHW and scores.dim() == 3 and self.channels == 1:
            scores = scores.unsqueeze(1)
        if scores.dim() != 4:
            raise RuntimeError(f"expected 4-D scores, got {tuple(scores.shape)}")
        if lay == L.SEG_NCHW:
            if scores.dtype not in _SCORE_ELEM:
                raise L.OctError(f"scores must be fp32, bf16 or uint8 (got {scores.dtype})")
            n, c, h, w = scores.shape
        else:
            if scores.dtype not in (torch.bfloat16, torch.float32):
                raise L.OctError(f"NHWC scores must be bf16 or fp32 (got {scores.dtype})")
            n, h, w, c = scores.shape
        if c != self.channels:
            raise RuntimeError(f"the scores have {c} channels, the evaluator {self.channels}")
        if h < 1 or w < 1:
            raise RuntimeError(f"scores need H, W >= 1, got {tuple(scores.shape)}")
        if n * c * h * w >= 2 ** 31:
            raise RuntimeError(f"one update takes fewer than 2^31 elements, got {n} x {c} x {h} x {w}")
        if scores.device.type != "cuda":
            raise L.OctError("the HIP path needs a device tensor (there is no CPU fallback)")
        target = _binary_target(target, n, c, h, w, scores.device)
        scores = scores.detach().contiguous()
        if lay == L.SEG_NHWC:
            planar = torch.empty((n, c, h, w), dtype=torch.float32, device=scores.device)
            if n:
                dt = L.DT_BF16 if scores.dtype == torch.bfloat16 else L.DT_F32
                L.check(L.lib().oct_nhwc_to_nchw(dt, scores.data_ptr(), planar.data_ptr(), n, c, h, w,
                                                 torch.cuda.current_stream(scores.device).cuda_stream), "oct_nhwc_to_nchw")
            scores = planar
        return self._launch(target, scores, n, h, w)

    @torch.no_grad()
    def update_model(self, model, x, target):
        """Forward of `model` in its current mode, then one update on its logits: the engine networks (UNet, BioUNet) through
        model.logits(x) (NCHW fp32), the logits networks (SegLossMixin) through their NHWC logits.  UNet3D is refused: the
        binary head is 2-D only."""
        ncls, logits_net = _model_kind(model)
        if not logits_net and not model._weighted_loss:
            raise NotImplementedError(f"{type(model).__name__}: the binary / multi-label head is implemented for the 2-D "
                                      "networks only")
        if ncls != self.channels:
            raise RuntimeError(f"{type(model).__name__} has {ncls} output channels, the evaluator {self.channels}")
        if not torch.is_tensor(x) or x.dim() != 4:
            raise RuntimeError(f"expected a batched input (B, C, H, W), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        want = (x.shape[0], ncls) + tuple(x.shape[2:])   # checked before the forward runs; update() applies the full rules
        if not torch.is_tensor(target) or tuple(target.shape) not in ((want, (want[0],) + want[2:]) if ncls == 1 else (want,)):
            raise RuntimeError(f"target must have shape {want}, got {tuple(target.shape) if torch.is_tensor(target) else type(target).__name__}")
        if logits_net:
            return self.update(target, model._run_logits(x), "nhwc")
        return self.update(target, model.logits(x), "nchw")

    def compute(self, thresholds=(0.5,)) -> dict:
        """The only call that synchronises: score_metrics_from_state on the state, thresholds as probabilities."""
        return score_metrics_from_state(self._host_state(), self.channels, thresholds, self.logits)

    def roc_curve(self, channel=0):
        """(fpr, tpr, thresholds) over the occupied keys in descending order; thresholds are key_value(key)"""
        r = score_curves_from_state(self._host_state(), self.channels, channel)
        return r["fpr"], r["tpr"], r["thresholds"]

    def pr_curve(self, channel=0):
        """(precision, recall, thresholds) over the occupied keys in descending order; thresholds are key_value(key)"""
        r = score_curves_from_state(self._host_state(), self.channels, channel)
        return r["precision"], r["tpr"], r["thresholds"]


# ---- lesion-wise scores: detection counts over connected components ----------------------------------------------------------
LESION_FIELDS = ("target_components", "pred_components", "detected", "confirmed")


def lesion_state_size(classes: int) -> int:
    return classes * len(LESION_FIELDS) + L.LESION_STATE_EXTRA


def _check_overlap(min_overlap):
    if not isinstance(min_overlap, (tuple, list)) or len(min_overlap) != 2:
        raise TypeError(f"min_overlap must be a pair of ints (num, den), got {min_overlap!r}")
    num, den = min_overlap
    for v in (num, den):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"min_overlap must be a pair of ints (num, den), got {min_overlap!r}")
    if not (1 <= den < 2 ** 31 and 0 <= num <= den):
        raise ValueError(f"min_overlap must be a fraction num / den in [0, 1] with 1 <= den < 2^31, got {num} / {den}")
    return num, den


def lesion_metrics_from_state(state, classes: int) -> dict:
    """The lesion-wise figures of LesionEvaluator from its int64 state (numpy float64, no GPU), per class:
      target_components, pred_components, detected, confirmed   int64 [C]
      sensitivity = detected / target_components, precision = confirmed / pred_components,
      f1 = 2 sensitivity precision / (sensitivity + precision)   float64 [C]; a 0 / 0 is NaN, f1 is NaN where either is NaN and 0
      where both are 0;   images, ignored, invalid, updates   int."""
    _check_config(classes, None)
    s = _int_state(state, lesion_state_size(classes), f"{classes} classes")
    counts = s[:classes * 4].reshape(classes, 4)
    nt, npred, det, conf = (counts[:, k].copy() for k in range(4))
    nan = np.float64("nan")
    sens = np.where(nt > 0, det / np.where(nt > 0, nt, 1), nan)
    prec = np.where(npred > 0, conf / np.where(npred > 0, npred, 1), nan)
    both = sens + prec                                     # NaN where either is
    f1 = np.where(both > 0, 2.0 * sens * prec / np.where(both > 0, both, 1.0), np.where(both == 0, 0.0, nan))
    images, ignored, invalid, updates = (int(v) for v in s[classes * 4:])
    return {"target_components": nt, "pred_components": npred, "detected": det, "confirmed": conf,
            "sensitivity": sens, "precision": prec, "f1": f1,
            "images": images, "ignored": ignored, "invalid": invalid, "updates": updates}


class LesionEvaluator(_StateEvaluator):
    """Lesion-wise detection scores of a validation set (csrc/components.hip, oct_lesion_eval_update): both maps are labelled
    into connected components (same value, 4- or 8-neighbours); a target component G of class c is DETECTED when
    inter(G) = #{pixels of G with pred == c} >= 1 and inter(G) * den >= num * area(G), num / den = min_overlap; a predicted
    component is CONFIRMED by the same rule with the roles swapped.  A pixel whose target equals ignore_index is outside in both
    maps, so it splits a predicted component that runs through it.  The int64 state is

        [classes][target_components, pred_components, detected, confirmed] | images | ignored | invalid | updates

    A batch goes through the kernels in chunks of images whose workspace (26 bytes per pixel) fits max_workspace_bytes."""

    def __init__(self, classes, connectivity=4, ignore_index=None, min_overlap=(0, 1), device=None, max_workspace_bytes=256 << 20):
        _check_config(classes, ignore_index)
        _check_connectivity(connectivity)
        _check_workspace_limit(max_workspace_bytes)
        self.min_overlap = _check_overlap(min_overlap)
        super().__init__(device, lesion_state_size(classes))
        self.classes = classes
        self.connectivity = connectivity
        self.ignore_index = ignore_index
        self.max_workspace_bytes = max_workspace_bytes
        self._workspace = None   # uint8 device buffer, grown on demand, reused by every update

    def _desc(self, images, h, w, target, pred):
        return L.CcDesc(images, h, w, self.classes, _elem(target), _elem(pred), self.connectivity, L.CC_OP_LESION,
                        int(self.ignore_index is not None), self.min_overlap[0], self.min_overlap[1], 0,
                        int(self.ignore_index or 0))

    def update(self, target, pred):
        """Two integer class maps of one shape (..., H, W), H, W <= 16384, with SegEvaluator.update's input rules.  One image
        whose workspace does not fit max_workspace_bytes raises.  Nothing is read back."""
        target, pred, (images, h, w) = _class_map_pair(target, pred, L.CC_MAX_DIM, "connected components")
        state = self._state_on(target.device)
        if images == 0:
            return self
        lib = L.lib()
        one = int(lib.oct_cc_workspace_bytes(C.byref(self._desc(1, h, w, target, pred))))
        if one == 0:
            raise L.OctError(f"oct_cc_workspace_bytes failed: {L.last_error()}")
        chunks = _image_chunks(images, h, w, one, self.max_workspace_bytes)
        target, pred = target.reshape(images, h, w), pred.reshape(images, h, w)
        stream = torch.cuda.current_stream(target.device).cuda_stream
        for lo, k in chunks:
            desc = self._desc(k, h, w, target, pred)
            need = int(lib.oct_cc_workspace_bytes(C.byref(desc)))
            self._workspace = _grown(self._workspace, need, target.device)
            L.check(lib.oct_lesion_eval_update(C.byref(desc), target[lo:lo + k].data_ptr(), pred[lo:lo + k].data_ptr(),
                                               state.data_ptr(), self._workspace.data_ptr(), stream), "oct_lesion_eval_update")
        return self

    @torch.no_grad()
    def update_model(self, model, x, target):
        """model.predict(x) of one of this package's networks in its current mode against target: the engine networks (UNet,
        BioUNet, UNet3D -- a (B, D, H, W) map counts B*D slice images) and the logits networks (SegLossMixin) alike."""
        ncls, _ = _model_kind(model)
        if ncls != self.classes:
            raise RuntimeError(f"{type(model).__name__} has {ncls} classes, the evaluator {self.classes}")
        return self.update(target, model.predict(x))

    def compute(self) -> dict:
        """The only call that synchronises: lesion_metrics_from_state on the state.  `updates` counts kernel calls, one per
        chunk of an update."""
        return lesion_metrics_from_state(self._host_state(), self.classes)


# ---- layer surfaces: boundary position error per surface -----------------------------------------------------------------------
SURFACE_FIELDS = ("count", "sum_abs", "sum_signed", "sum_sq", "max_abs")


def surface_state_size(surfaces: int) -> int:
    return surfaces * len(SURFACE_FIELDS)


def surface_metrics_from_state(state, surfaces: int) -> dict:
    """The boundary position errors of SurfaceEvaluator from its int64 state [surfaces][count, sum |e|, sum e, sum e^2, max |e|]
    (numpy float64, no GPU), e = predicted - target row in pixels, per surface:
      columns int64;  mean_abs_error = sum |e| / columns, mean_signed_error = sum e / columns (positive: predicted too deep),
      rmse = sqrt(sum e^2 / columns), max_abs_error -- NaN where a surface has no column;
      mean_mean_abs_error, mean_mean_signed_error, mean_rmse, mean_max_abs_error: their means over the surfaces that have
      columns (NaN without one)."""
    _check_int("surfaces", surfaces, 1, L.SURF_MAX_K - 1)
    s = _int_state(state, surface_state_size(surfaces), f"{surfaces} surfaces").reshape(surfaces, len(SURFACE_FIELDS))
    n = s[:, 0].copy()
    has = n > 0
    den = np.where(has, n, 1).astype(np.float64)
    nan = np.float64("nan")
    res = {
        "columns": n,
        "mean_abs_error": np.where(has, s[:, 1] / den, nan),
        "mean_signed_error": np.where(has, s[:, 2] / den, nan),
        "rmse": np.where(has, np.sqrt(s[:, 3] / den), nan),
        "max_abs_error": np.where(has, s[:, 4].astype(np.float64), nan),
    }
    for k in ("mean_abs_error", "mean_signed_error", "rmse", "max_abs_error"):
        res["mean_" + k] = float(res[k][has].mean()) if has.any() else float("nan")
    return res


class SurfaceEvaluator(_StateEvaluator):
    """Boundary position error per layer surface -- mean absolute, signed and RMS, in pixels: the headline number of the
    layer-segmentation papers -- accumulated on the device (csrc/surfaces.hip, oct_surf_error_update).  The int64 state is

        [surfaces][count, sum |e|, sum e, sum e^2, max |e|],   e = predicted - target row, over the valid columns

        layers = LayerSurfaces(classes=9, order=range(8), max_step=1, ignore_index=255)
        ev = SurfaceEvaluator(surfaces=7)
        for x, y in loader:
            ev.update_maps(y, model.predict(x), layers)     # or ev.update(target_surfaces, layers.from_model(model, x))
        m = ev.compute()                                    # the one synchronisation; m["mean_abs_error"], m["rmse"], ..."""

    def __init__(self, surfaces, device=None):
        _check_int("surfaces", surfaces, 1, L.SURF_MAX_K - 1)
        super().__init__(device, surface_state_size(surfaces))
        self.surfaces = surfaces

    def update(self, target_surfaces, pred_surfaces, valid=None):
        """Two int32 surface tensors of one shape (..., surfaces, W) -- what LayerSurfaces.extract returns -- and optionally
        `valid` (..., W), bool / uint8: the columns that count (all of them without it).  The rows are expected in
        [0, 4095], the range extract writes: the int64 sums are then exact.  The values stay on the device and are not
        range-checked (that would synchronise); rows made up with |e| near 2^32 would wrap the sum of squares."""
        from .surfaces import _check_surfaces
        if not torch.is_tensor(target_surfaces):
            raise TypeError(f"target_surfaces must be a torch tensor, got {type(target_surfaces).__name__}")
        if target_surfaces.dim() < 2 or target_surfaces.shape[-2] != self.surfaces or target_surfaces.shape[-1] < 1:
            raise RuntimeError(f"target_surfaces must have shape (..., {self.surfaces}, W >= 1), got {tuple(target_surfaces.shape)}")
        w = target_surfaces.shape[-1]
        images = target_surfaces.numel() // (self.surfaces * w)
        device = target_surfaces.device
        t = _check_surfaces(target_surfaces, images, self.surfaces + 1, w, device, "target_surfaces")
        p = _check_surfaces(pred_surfaces, images, self.surfaces + 1, w, device, "pred_surfaces")
        if valid is not None:
            if not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8):
                raise TypeError("valid must be a bool / uint8 tensor, got "
                                f"{valid.dtype if torch.is_tensor(valid) else type(valid).__name__}")
            if valid.numel() != images * w or valid.shape[-1] != w:
                raise RuntimeError(f"valid must have shape (..., {w}) for {images} images, got {tuple(valid.shape)}")
            if valid.device != device:
                raise RuntimeError(f"valid is on {valid.device}, the surfaces on {device}")
            valid = valid.to(torch.uint8).contiguous()
        state = self._state_on(device)
        if images == 0:
            return self
        desc = L.SurfDesc(images, 1, w, 1, 0, self.surfaces + 1, -1, 0, 0, 1, 1.0, 0, 0)
        L.check(L.lib().oct_surf_error_update(C.byref(desc), t.data_ptr(), p.data_ptr(), L.ptr(valid), state.data_ptr(),
                                              torch.cuda.current_stream(device).cuda_stream), "oct_surf_error_update")
        return self

    def update_maps(self, target_map, pred_map, extractor):
        """Two integer class maps of one shape (..., H, W) through `extractor` (a LayerSurfaces over surfaces + 1 classes): the
        predicted surfaces with its settings, the target's with max_step=None -- for a topologically valid target exactly its
        boundaries.  With the extractor's ignore_index a column counts where any of its target pixels is not ignore_index."""
        from .surfaces import LayerSurfaces
        if not isinstance(extractor, LayerSurfaces):
            raise TypeError(f"extractor must be a LayerSurfaces, got {type(extractor).__name__}")
        if len(extractor.order) != self.surfaces + 1:
            raise RuntimeError(f"the extractor orders {len(extractor.order)} classes, the evaluator has {self.surfaces} surfaces")
        target_map, pred_map, _ = _class_map_pair(target_map, pred_map)
        valid = None
        if extractor.ignore_index is not None:
            valid = (target_map != extractor.ignore_index).any(-2)
        return self.update(extractor.unconstrained().extract(target_map), extractor.extract(pred_map), valid)

    def all_reduce(self, group=None):
        """Sum the counts and sums over the ranks of `group` and take the maximum of max |e| (a SUM and a MAX all-reduce)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if self.state is None:
            self._state_on(self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device()))
        rows = self.state.view(self.surfaces, len(SURFACE_FIELDS))
        worst = rows[:, 4].clone()
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(worst, op=dist.ReduceOp.MAX, group=group)
        rows[:, 4] = worst
        return self

    def compute(self) -> dict:
        """The only call that synchronises: surface_metrics_from_state on the state."""
        return surface_metrics_from_state(self._host_state(), self.surfaces)
