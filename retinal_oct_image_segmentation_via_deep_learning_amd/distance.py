"""Distance maps of class maps on the device (csrc/distance.hip): the exact Euclidean distance transform, the boundary weight
maps of a weighted loss and the signed distance maps of a boundary loss.

Every pixel-weight scheme of retinal-layer work is a function of the distance to a label boundary: ReLayNet's bonus on the
boundary pixels, U-Net's 1 + w0 exp(-d^2 / 2 sigma^2), Kervadec's signed distance maps.  The place to compute one is AFTER the
augmentation, on the augmented labels, where they lie -- no scipy.ndimage.distance_transform_edt per image and class, no
upload, and no bilinear warp that blurs a map made before it.

  valid     a pixel whose value is in [0, classes) and is not ignore_index.  An invalid pixel is a site of no plane; it still
            receives a distance
  planes    "boundary"    valid pixels with a 4-neighbour inside the image that is valid and has another value (the image edge
                          is no boundary, an ignored neighbour makes none)
            ("class", c)  valid pixels equal to c          ("other", c)  valid pixels not equal to c
  D2        int32: the exact squared distance in pixels to the nearest site of the plane in the image; 0 on a site, FAR = 2^30
            everywhere in an image whose plane has no site

    wmap = DistanceWeightMap.gaussian(classes=9, w0=10.0, sigma=5.0, ignore_index=label_fill)
    img, tgt = augmenter(...)
    w = wmap(tgt)                                      # fp32 (B, H, W), no synchronisation
    model.forward_backward(img, tgt, pixel_weight=w, ignore_index=label_fill)

The weight is table[min(D2, len(table) - 1)]: a table indexed by the SQUARED distance, so any profile of the distance tabulated
on the host in float64 and rounded once is reproduced bit for bit.  Integers up to that lookup: two runs give the same bits.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .evaluation import _check_config, _check_int, _class_map, _elem, _grown, _map_geometry
from .postprocess import _need_device

FAR = L.DT_FAR
_KINDS = {"boundary": L.DT_BOUNDARY, "class": L.DT_CLASS, "other": L.DT_OTHER}


def block():
    """(rows one column-pass thread covers, pixels one row-pass workgroup covers where rows are shorter than that)"""
    rows, cols = C.c_int(0), C.c_int(0)
    L.check(L.lib().oct_dt_block(C.byref(rows), C.byref(cols)), "oct_dt_block")
    return rows.value, cols.value


def _check_planes(planes, classes):
    """the plane list as [(kind code, class)]: "boundary", ("class", c), ("other", c)"""
    if isinstance(planes, str) or not isinstance(planes, (list, tuple)):
        raise TypeError(f"planes must be a sequence of 'boundary', ('class', c), ('other', c), got {planes!r}")
    if not planes:
        raise ValueError("planes is empty: name at least one of 'boundary', ('class', c), ('other', c)")
    if len(planes) > L.DT_MAX_PLANES:
        raise ValueError(f"one call takes at most {L.DT_MAX_PLANES} planes, got {len(planes)}")
    out = []
    for p in planes:
        if p == "boundary":
            out.append((L.DT_BOUNDARY, 0))
            continue
        if not isinstance(p, (list, tuple)) or len(p) != 2 or p[0] not in ("class", "other"):
            raise ValueError(f"a plane is 'boundary', ('class', c) or ('other', c), got {p!r}")
        _check_int(f"the class of plane {p!r}", p[1], 0, classes - 1)
        out.append((_KINDS[p[0]], p[1]))
    return out


def _check_class_ids(class_ids, classes):
    ids = list(range(classes)) if class_ids is None else class_ids
    if not isinstance(ids, (list, tuple)):
        raise TypeError(f"class_ids must be a sequence of ints or None, got {type(ids).__name__}")
    if not ids:
        raise ValueError("class_ids is empty")
    if len(ids) > L.DT_MAX_PLANES // 2:
        raise ValueError(f"one call takes at most {L.DT_MAX_PLANES // 2} classes, got {len(ids)}")
    for c in ids:
        _check_int("class_ids entries", c, 0, classes - 1)
    return list(ids)


def _geometry(m):
    """a class map as the kernels read it and (images, h, w)"""
    m = _class_map(m, "map")
    images, h, w = _map_geometry(m, L.DT_MAX_DIM, "distance maps")
    if images * h * w >= 2 ** 31:
        raise RuntimeError(f"one call takes fewer than 2^31 pixels, got {images} x {h} x {w}")
    return m, images, h, w


def _desc(images, h, w, classes, m, ignore_index, nplanes, op):
    return L.DtDesc(images, h, w, classes, _elem(m), int(ignore_index is not None), nplanes, op, int(ignore_index or 0))


def _workspace_bytes(desc):
    need = int(L.lib().oct_dt_workspace_bytes(C.byref(desc)))
    if need == 0:
        raise L.OctError(f"oct_dt_workspace_bytes failed: {L.last_error()}")
    return need


def _plane_array(pairs):
    flat = [v for pair in pairs for v in pair]
    return (C.c_int32 * len(flat))(*flat)


def _stream(m):
    return torch.cuda.current_stream(m.device).cuda_stream


def _out(m, nplanes, dtype):
    h, w = m.shape[-2:]
    return torch.empty(tuple(m.shape[:-2]) + (nplanes, h, w), dtype=dtype, device=m.device)


def squared_distance(map, classes, planes, ignore_index=None):
    """int32 (*lead, P, H, W): the exact squared Euclidean distance of every pixel of the integer class map (*lead, H, W) to the
    nearest site of each of the P planes (module doc-string), FAR where an image has no site of the plane.  uint8 and int64
    are read as they are, other integer dtypes are converted to int64.  No synchronisation; no CPU fallback."""
    _check_config(classes, ignore_index)
    pairs = _check_planes(planes, classes)
    m, images, h, w = _geometry(map)
    _need_device(m)
    out = _out(m, len(pairs), torch.int32)
    if images:
        desc = _desc(images, h, w, classes, m, ignore_index, len(pairs), L.DT_OP_SQUARED)
        ws = torch.empty(_workspace_bytes(desc), dtype=torch.uint8, device=m.device)
        L.check(L.lib().oct_dt_squared(C.byref(desc), _plane_array(pairs), m.data_ptr(), out.data_ptr(), ws.data_ptr(), _stream(m)),
                "oct_dt_squared")
    return out


def signed_distance(map, classes, class_ids=None, ignore_index=None):
    """fp32 (*lead, K, H, W), one plane per entry c of class_ids (default: every class): -sqrt(D2 to ("other", c)) on a pixel of
    class c, +sqrt(D2 to ("class", c)) on every other pixel -- negative inside, positive outside, never 0 where both sides
    exist.  The whole plane of an image is 0 when the class is absent or nothing valid lies outside it (Kervadec's
    convention).  One IEEE square root per pixel.  It feeds a boundary-loss term written in torch on model(x):
    (softmax(logits, 1)[:, class_ids] * signed_distance(t, classes, class_ids)).mean().  No synchronisation."""
    _check_config(classes, ignore_index)
    ids = _check_class_ids(class_ids, classes)
    m, images, h, w = _geometry(map)
    _need_device(m)
    out = _out(m, len(ids), torch.float32)
    if images:
        desc = _desc(images, h, w, classes, m, ignore_index, len(ids), L.DT_OP_SIGNED)
        ws = torch.empty(_workspace_bytes(desc), dtype=torch.uint8, device=m.device)
        L.check(L.lib().oct_dt_signed(C.byref(desc), (C.c_int32 * len(ids))(*ids), m.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                      _stream(m)), "oct_dt_signed")
    return out


def _check_float(name, value, lo=None):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
        raise TypeError(f"{name} must be a finite number, got {value!r}")
    if lo is not None and not value > lo:
        raise ValueError(f"{name} must be above {lo}, got {value}")
    return float(value)


class DistanceWeightMap:
    """The pixel-weight map of a weighted loss from the labels of the step: called on an integer class map (B, H, W) it returns
    the contiguous fp32 tensor (B, H, W) on the map's device that `pixel_weight=` takes,

        weight = table[min(D2, len(table) - 1)],   D2 = squared distance to the nearest "boundary" pixel (module doc-string)

    `table` is any float sequence or tensor, converted to fp32 ONCE; its last entry is the weight far from every boundary, and
    of an image without one.  The workspace is cached and grown; nothing synchronises; there is no CPU fallback.

        wmap = DistanceWeightMap.gaussian(classes=9, w0=10.0, sigma=5.0, ignore_index=label_fill)
        img, tgt = augmenter(...)
        w = wmap(tgt)
        model.forward_backward(img, tgt, pixel_weight=w, ignore_index=label_fill)
    """

    def __init__(self, classes, table, ignore_index=None):
        _check_config(classes, ignore_index)
        if torch.is_tensor(table):
            t = table.detach().to("cpu", torch.float64).reshape(-1)
        else:
            if isinstance(table, (str, bytes)) or not hasattr(table, "__len__"):
                raise TypeError(f"table must be a sequence of floats or a tensor, got {type(table).__name__}")
            t = torch.from_numpy(np.asarray(table, dtype=np.float64).reshape(-1).copy())
        if t.numel() == 0:
            raise ValueError("table is empty: it needs at least the weight far from every boundary")
        if t.numel() >= 2 ** 31:
            raise ValueError(f"table must have fewer than 2^31 entries, got {t.numel()}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("table must hold finite weights")
        self.classes = classes
        self.ignore_index = ignore_index
        self.table = t.to(torch.float32)   # host copy: the one rounding
        self._device_table = {}            # device -> the table there
        self._workspace = None             # uint8 device buffer, grown on demand, reused by every call
        self._planes = _plane_array([(L.DT_BOUNDARY, 0)])

    @classmethod
    def gaussian(cls, classes, w0, sigma, base=1.0, cutoff_sigmas=4.0, ignore_index=None):
        """U-Net's scheme: weight = base + w0 exp(-d^2 / (2 sigma^2)) up to d = ceil(cutoff_sigmas * sigma), `base` beyond:
        table[k] = base + w0 exp(-k / (2 sigma^2)) for k = 0 .. ceil(cutoff_sigmas * sigma)^2 in float64, then one entry `base`"""
        w0, base = _check_float("w0", w0), _check_float("base", base)
        sigma, cutoff_sigmas = _check_float("sigma", sigma, 0), _check_float("cutoff_sigmas", cutoff_sigmas, 0)
        kmax = math.ceil(cutoff_sigmas * sigma) ** 2
        if kmax + 2 >= 2 ** 31:
            raise ValueError(f"cutoff_sigmas * sigma = {cutoff_sigmas * sigma} needs a table of {kmax + 2} entries")
        k = np.arange(kmax + 1, dtype=np.float64)
        table = np.concatenate([base + w0 * np.exp(-k / (2.0 * sigma * sigma)), [base]])
        return cls(classes, table, ignore_index)

    @classmethod
    def boundary_bonus(cls, classes, w1, base=1.0, ignore_index=None):
        """ReLayNet's term: base + w1 on the boundary pixels, base everywhere else: table = [base + w1, base]"""
        w1, base = _check_float("w1", w1), _check_float("base", base)
        return cls(classes, [base + w1, base], ignore_index)

    def _table_on(self, device):
        t = self._device_table.get(device)
        if t is None:
            t = self._device_table[device] = self.table.to(device)
        return t

    def __call__(self, map):
        m, images, h, w = _geometry(map)
        _need_device(m)
        out = torch.empty(m.shape, dtype=torch.float32, device=m.device)
        if images == 0:
            return out
        table = self._table_on(m.device)
        desc = _desc(images, h, w, self.classes, m, self.ignore_index, 1, L.DT_OP_WEIGHT)
        ws = self._workspace = _grown(self._workspace, _workspace_bytes(desc), m.device)
        L.check(L.lib().oct_dt_weight_map(C.byref(desc), self._planes, m.data_ptr(), table.data_ptr(), table.numel(), out.data_ptr(),
                                          ws.data_ptr(), _stream(m)), "oct_dt_weight_map")
        return out
