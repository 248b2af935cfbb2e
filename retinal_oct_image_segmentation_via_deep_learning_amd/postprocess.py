"""Connected components of class maps on the device (csrc/components.hip): labelling, a component table and a cleanup filter.

Between `model.predict(x)` / `predict_mask(x)` and the evaluators sits the step that knows what an *object* is: drop fluid
specks below a minimum area, keep the largest component of each retinal layer, fill the holes of a mask.  All of it is one
kernel family on the map where it lies -- no `prediction.cpu()`, no scipy.ndimage.label per image and class.

  outside    a pixel whose value is not in [0, classes), or equals ignore_index
  connected  two inside pixels with the SAME value that are 4-neighbours (connectivity=4) or 8-neighbours (connectivity=8): one
             pass labels every class, and the background's components (the "holes") come with it
  roots      int32, the map's shape: the smallest y*W + x of the pixel's component, -1 outside.  Ascending root order per class
             is scipy.ndimage.label's numbering
  info       int32, the map's shape: area | touches_border << 30 at a root pixel, 0 elsewhere; touches_border = some pixel of
             the component lies in the first or last row or column

    flt = ComponentFilter(classes=9, min_area=[0, 0, 0, 0, 0, 0, 0, 0, 20], keep_largest=[0, 1, 1, 1, 1, 1, 1, 1, 0])
    clean = flt(model.predict(x))                      # no synchronisation
    holes = ComponentFilter(2, fill_enclosed=[1, 0], replace=[1, 0])      # background enclosed by the mask becomes mask
    masks = holes.filter_masks(model.predict_mask(x))

The filter is ONE pass over the components of its input: a component is replaced when its area is below min_area[c], or
keep_largest[c] is set and it is not the largest of its class in the image (ties: the smallest root), or fill_enclosed[c] is set
and it does not touch the image border.  What a replacement merges or uncovers is not looked at again.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .evaluation import _check_config, _check_connectivity, _class_map, _elem, _grown, _map_geometry

AREA_MASK = (1 << L.CC_BORDER_BIT) - 1


def tile():
    """(rows, columns) of the tile one workgroup labels in LDS"""
    th, tw = C.c_int(0), C.c_int(0)
    L.check(L.lib().oct_cc_tile(C.byref(th), C.byref(tw)), "oct_cc_tile")
    return th.value, tw.value


def _geometry(m, what="map"):
    """a class map as the kernels read it and (images, h, w)"""
    m = _class_map(m, what)
    images, h, w = _map_geometry(m, L.CC_MAX_DIM, "connected components")
    if images * h * w >= 2 ** 31:
        raise RuntimeError(f"one call takes fewer than 2^31 pixels, got {images} x {h} x {w}")
    return m, images, h, w


def _need_device(m):
    if m.device.type != "cuda":
        raise L.OctError("the HIP path needs a device tensor (there is no CPU fallback)")


def _desc(images, h, w, classes, m, connectivity, ignore_index, op, pred=None, min_overlap=(0, 1)):
    return L.CcDesc(images, h, w, classes, _elem(m), 0 if pred is None else _elem(pred), connectivity, op,
                    int(ignore_index is not None), min_overlap[0], min_overlap[1], 0, int(ignore_index or 0))


def _workspace_bytes(desc, what):
    need = int(L.lib().oct_cc_workspace_bytes(C.byref(desc)))
    if need == 0:
        raise L.OctError(f"oct_cc_workspace_bytes failed for {what}: {L.last_error()}")
    return need


def _label(m, images, h, w, classes, connectivity, ignore_index, workspace, op=L.CC_OP_LABEL):
    roots = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    info = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    if images:
        desc = _desc(images, h, w, classes, m, connectivity, ignore_index, op)
        L.check(L.lib().oct_cc_label(C.byref(desc), m.data_ptr(), roots.data_ptr(), info.data_ptr(), workspace.data_ptr(),
                                     torch.cuda.current_stream(m.device).cuda_stream), "oct_cc_label")
    return roots, info


def connected_components(map, classes, connectivity=4, ignore_index=None):
    """(roots, info) of an integer class map (..., H, W) on the device, both int32 of the map's shape (module doc-string).  uint8
    and int64 are read as they are, other integer dtypes are converted to int64; every leading dimension counts images.  No
    synchronisation."""
    _check_config(classes, ignore_index)
    _check_connectivity(connectivity)
    m, images, h, w = _geometry(map)
    _need_device(m)
    ws = None
    if images:
        need = _workspace_bytes(_desc(images, h, w, classes, m, connectivity, ignore_index, L.CC_OP_LABEL), "the labelling")
        ws = torch.empty(need, dtype=torch.uint8, device=m.device)
    return _label(m, images, h, w, classes, connectivity, ignore_index, ws)


def component_table(map, classes, connectivity=4, ignore_index=None):
    """int64 [n, 6] on the device: one row (image, class, root_y, root_x, area, touches_border) per component, sorted by image,
    class and root -- per class the order of scipy.ndimage.label.  Built with torch ops on `info`; the number of rows is not
    known before the labelling has run, so THIS CALL SYNCHRONISES with the device (torch.nonzero); it is the one call of this
    module that does."""
    roots, info = connected_components(map, classes, connectivity, ignore_index)
    h, w = info.shape[-2:]
    flat = info.reshape(-1, h * w)
    pos = torch.nonzero(flat)                               # the synchronisation; rows sorted by (image, root)
    img, root = pos[:, 0], pos[:, 1]
    v = flat[img, root].to(torch.int64)
    cls = map.reshape(-1, h * w)[img, root].to(torch.int64)
    order = torch.argsort((img * classes + cls) * (h * w) + root)
    rows = torch.stack([img, cls, root // w, root % w, v & AREA_MASK, v >> L.CC_BORDER_BIT], dim=1)
    return rows[order]


def _per_class(value, classes, name, lo, hi):
    """a scalar or a per-class sequence as a list of `classes` ints in [lo, hi]"""
    if value is None:
        return [0] * classes
    seq = list(value) if isinstance(value, (list, tuple)) else [value] * classes
    if len(seq) != classes:
        raise ValueError(f"{name} must be a scalar or have one entry per class ({classes}), got {len(seq)}")
    out = []
    for v in seq:
        if isinstance(v, bool):
            v = int(v)
        if not isinstance(v, int):
            raise TypeError(f"{name} must hold ints, got {type(v).__name__} {v!r}")
        if not lo <= v <= hi:
            raise ValueError(f"{name} entries must be in [{lo}, {hi}], got {v}")
        out.append(v)
    return out


class ComponentFilter:
    """The cleanup filter of the module doc-string.  Each rule is a scalar (every class) or a per-class sequence:
      min_area       components with fewer pixels are replaced (0 / None: off; area == min_area is kept)
      keep_largest   0 / 1: all but the image's largest component of the class are replaced (ties: the smallest root)
      fill_enclosed  0 / 1: components of the class that do not touch the image border are replaced
      replace        the value replaced pixels of the class get (any int64; 0..255 is what fits a uint8 map)
    The workspace is cached and grown; nothing synchronises; there is no CPU fallback."""

    def __init__(self, classes, min_area=None, keep_largest=None, fill_enclosed=None, replace=0, connectivity=4, ignore_index=None):
        _check_config(classes, ignore_index)
        _check_connectivity(connectivity)
        self.classes = classes
        self.connectivity = connectivity
        self.ignore_index = ignore_index
        self.min_area = _per_class(min_area, classes, "min_area", 0, 2 ** 31 - 1)
        self.keep_largest = _per_class(keep_largest, classes, "keep_largest", 0, 1)
        self.fill_enclosed = _per_class(fill_enclosed, classes, "fill_enclosed", 0, 1)
        self.replace = _per_class(replace, classes, "replace", -2 ** 63, 2 ** 63 - 1)
        self._rules = L.CcRules()
        for c in range(classes):
            self._rules.min_area[c] = self.min_area[c]
            self._rules.keep_largest[c] = self.keep_largest[c]
            self._rules.drop_enclosed[c] = self.fill_enclosed[c]
            self._rules.replace[c] = self.replace[c]
        self._workspace = None   # uint8 device buffer, grown on demand, reused by every call

    def __call__(self, map, out=None):
        """The filtered map: the input's shape and (after the conversion of connected_components) dtype.  `out` may be a
        tensor of that shape and dtype to write into -- the converted input itself for a filter in place."""
        m, images, h, w = _geometry(map)
        if m.dtype == torch.uint8 and any(not 0 <= r <= 255 for r in self.replace):
            raise ValueError(f"replace {self.replace} does not fit a uint8 map")
        _need_device(m)
        if out is None:
            out = torch.empty_like(m)
        elif not torch.is_tensor(out) or out.shape != m.shape or out.dtype != m.dtype or out.device != m.device or \
                not out.is_contiguous():
            raise RuntimeError(f"out must be a contiguous {m.dtype} tensor of shape {tuple(m.shape)} on {m.device}")
        if images == 0:
            return out
        desc = _desc(images, h, w, self.classes, m, self.connectivity, self.ignore_index, L.CC_OP_FILTER)
        ws = self._workspace = _grown(self._workspace, _workspace_bytes(desc, "the filter"), m.device)
        roots, info = _label(m, images, h, w, self.classes, self.connectivity, self.ignore_index, ws, L.CC_OP_FILTER)
        L.check(L.lib().oct_cc_filter(C.byref(desc), C.byref(self._rules), m.data_ptr(), roots.data_ptr(), info.data_ptr(),
                                      out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(m.device).cuda_stream),
                "oct_cc_filter")
        return out

    def filter_masks(self, mask):
        """The uint8 (B, C, H, W) output of predict_mask as B*C two-class images (0 background, 1 mask), every channel under
        the same rules: the filter must have been made with classes=2."""
        if self.classes != 2:
            raise RuntimeError(f"filter_masks takes a two-class filter (0 background, 1 mask), this one has {self.classes} classes")
        if not torch.is_tensor(mask) or mask.dim() != 4 or mask.dtype not in (torch.uint8, torch.bool):
            raise RuntimeError("filter_masks takes a uint8 mask of shape (B, C, H, W), got "
                               f"{(mask.dtype, tuple(mask.shape)) if torch.is_tensor(mask) else type(mask).__name__}")
        return self(mask)
