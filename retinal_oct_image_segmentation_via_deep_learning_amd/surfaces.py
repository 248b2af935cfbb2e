"""Layer surfaces on the device (csrc/surfaces.hip): ordered, smooth boundary rows from a class map or from a network's scores.

A layer network is judged by its *surfaces*: one boundary row per A-scan and interface, ordered top to bottom, no holes, no
islands.  An arg-max map guarantees none of that.  The classical repair is graph search: one shortest path per surface with a
smoothness limit between neighbouring A-scans.  Here it runs on the map (or the logits) where they lie, in exact integers -- no
`prediction.cpu()`, no Python loop per image and surface -- and two runs give the same bits.

Inputs
  a class map (..., H, W), uint8 / int64 (other integer dtypes are converted to int64), or scores (B, C, H, W), NCHW fp32 / bf16
  (`model.logits(x)` returns the fp32 form); H <= 4095
  order      K distinct classes, top to bottom, 2 <= K <= 16
  max_step   None, or an integer in [0, 32]: the most a surface moves between neighbouring columns
  scale, qmax   scores only: fp32 finite > 0 (default 16) and 1..255 (default 255)
Free pixels
  map: the value is not in `order`, equals ignore_index or lies outside [0, classes).  scores: any channel is NaN.
  A free pixel costs nothing wherever a surface passes.
Unary cost u_j(y, x), j = 0..K-1
  map: 0 if the pixel is free or its class is order[j], else 1
  scores: m = the maximum over all C channels; v = (m - z[order[j]]) * scale + 0.5, every operation rounded separately in fp32
  with no FMA contraction, the difference taken as 0 where z == m; u_j = floor(v) if v < qmax + 1, else qmax.  bf16 is
  widened to fp32 first
Surface k (k = 1..K-1) splits the groups order[:k] | order[k:]
  d_k(y, x) = min_{j<k} u_j - min_{j>=k} u_j;   N_k(x, s) = sum_{y<s} d_k(y, x) for s = 0..H -- the rows y < s lie above it
Path
  the path s_k(0..W-1) with |s_k(x+1) - s_k(x)| <= max_step that minimises sum_x N_k(x, s_k(x)), chosen by exactly this
  recurrence:  A(0, s) = N(0, s);  A(x, s) = N(x, s) + min A(x-1, t) over |t - s| <= max_step, 0 <= t <= H;  P(x, s) is the
  SMALLEST such t;  s(W-1) is the smallest argmin of A(W-1, .);  s(x-1) = P(x, s(x)).
  With max_step = None, s(x) is the smallest argmin of N(x, .).
  Afterwards s_k <- max(s_k, s_{k-1}) down the surfaces: N_{k+1} - N_k is non-increasing in s, so the minimisers are ordered
  by themselves and this step only breaks ties
Outputs
  surfaces   int32 (B, K-1, W), values in [0, H]
  painted    the input map's dtype, int64 for scores: out(y, x) = order[#{k : s_k(x) <= y}].  A pixel keeps its input class if
             that class is listed in `keep` (disjoint from `order`) -- how a fluid class survives; for scores the input class is
             the arg-max (first maximum, the first NaN beats everything: model.predict's rule)
Refused
  qmax * H * W >= 2^31 (a map counts as qmax = 1; every path cost then fits int32) and H > 4095: RuntimeError

    layers = LayerSurfaces(classes=9, order=range(8), max_step=1, keep=(8,))
    s = layers.from_model(model, x)                    # int32 (B, 7, W), no synchronisation
    clean = layers.paint(model.logits(x), s)           # a topologically valid int64 map, fluid (class 8) kept
    ev = SurfaceEvaluator(surfaces=7)
    ev.update_maps(target, model.predict(x), layers)   # boundary position error per surface
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from .evaluation import _check_config, _check_int, _check_workspace_limit, _class_map, _elem, _grown, _image_chunks, _map_geometry
from .postprocess import _need_device

MAX_K, MAX_H, MAX_STEP = L.SURF_MAX_K, L.SURF_MAX_H, L.SURF_MAX_STEP


def _check_order(order, classes, keep=()):
    """(order, keep) as lists of ints: 2..16 distinct classes, keep disjoint from them"""
    out = []
    for name, seq in (("order", order), ("keep", keep)):
        if isinstance(seq, range):
            seq = list(seq)
        if isinstance(seq, (str, bytes)) or not isinstance(seq, (list, tuple)):
            raise TypeError(f"{name} must be a sequence of ints, got {type(seq).__name__}")
        for c in seq:
            _check_int(f"{name} entries", c, 0, classes - 1)
        if len(set(seq)) != len(seq):
            raise ValueError(f"{name} names a class twice: {list(seq)}")
        out.append(list(seq))
    order, keep = out
    if not 2 <= len(order) <= MAX_K:
        raise ValueError(f"order must name 2..{MAX_K} classes, got {len(order)}")
    if set(order) & set(keep):
        raise ValueError(f"keep must be disjoint from order, both name {sorted(set(order) & set(keep))}")
    return order, keep


def _check_path_costs(qmax, h, w):
    if h > MAX_H:
        raise RuntimeError(f"layer surfaces take H <= {MAX_H}, got {h}")
    if qmax * h * w >= 2 ** 31:
        raise RuntimeError(f"qmax * H * W must stay below 2^31 (int32 path costs), got {qmax} x {h} x {w}")


def _check_surfaces(surfaces, images, k, w, device, what="surfaces"):
    if not torch.is_tensor(surfaces):
        raise TypeError(f"{what} must be a torch tensor, got {type(surfaces).__name__}")
    if surfaces.dtype != torch.int32:
        raise TypeError(f"{what} must be int32, got {surfaces.dtype}")
    if surfaces.dim() < 2 or tuple(surfaces.shape[-2:]) != (k - 1, w) or surfaces.numel() != images * (k - 1) * w:
        raise RuntimeError(f"{what} must have shape (..., {k - 1}, {w}) for {images} images, got {tuple(surfaces.shape)}")
    if surfaces.device != device:
        raise RuntimeError(f"{what} is on {surfaces.device}, the input on {device}")
    return surfaces.contiguous()


class LayerSurfaces:
    """The extractor of the module doc-string.  `extract` / `extract_scores` return the int32 surfaces (*lead, K-1, W), `paint`
    the valid map they describe, `__call__(map)` is extract followed by paint, `from_model(model, x)` extracts from
    model.logits(x).  With max_step set, a batch goes through the kernels in chunks of images whose workspace (about
    5 (K-1) W (H+1) bytes an image) fits max_workspace_bytes; the workspace is cached and grown.  Nothing synchronises; there
    is no CPU fallback."""

    def __init__(self, classes, order, max_step=1, keep=(), ignore_index=None, scale=16.0, qmax=255, max_workspace_bytes=256 << 20):
        _check_config(classes, ignore_index)
        self.order, self.keep = _check_order(order, classes, keep)
        _check_int("max_step", max_step, 0, MAX_STEP, True)
        if isinstance(scale, bool) or not isinstance(scale, (int, float)):
            raise TypeError(f"scale must be a number, got {type(scale).__name__} {scale!r}")
        scale32 = torch.tensor(float(scale), dtype=torch.float32).item()   # what the kernel multiplies by
        if not (math.isfinite(scale32) and scale32 > 0):
            raise ValueError(f"scale must be finite and positive in fp32, got {scale!r}")
        _check_int("qmax", qmax, 1, 255)
        _check_workspace_limit(max_workspace_bytes)
        self.classes = classes
        self.max_step = max_step
        self.ignore_index = ignore_index
        self.scale = scale32
        self.qmax = qmax
        self.max_workspace_bytes = max_workspace_bytes
        self._order = (C.c_int32 * len(self.order))(*self.order)
        self._keep = (C.c_int32 * max(1, len(self.keep)))(*self.keep)
        self._workspace = None   # uint8 device buffer, grown on demand, reused by every call
        self._free = None        # unconstrained(), made once

    def unconstrained(self):
        """the same settings with max_step=None (this extractor itself if it has none): on a topologically valid map its
        surfaces are exactly the boundaries"""
        if self.max_step is None:
            return self
        if self._free is None:
            self._free = LayerSurfaces(self.classes, self.order, None, self.keep, self.ignore_index, self.scale, self.qmax,
                                       self.max_workspace_bytes)
        return self._free

    # ---- inputs -------------------------------------------------------------------------------------------------------------
    def _map(self, m):
        if torch.is_tensor(m) and m.dim() >= 2:
            _check_path_costs(1, *m.shape[-2:])   # before _class_map makes a contiguous copy
        m = _class_map(m, "map")
        return (m,) + _map_geometry(m)

    def _scores(self, z):
        if not torch.is_tensor(z):
            raise TypeError(f"scores must be a torch tensor, got {type(z).__name__}")
        if z.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"scores must be fp32 or bf16, got {z.dtype}")
        if z.dim() != 4:
            raise RuntimeError(f"scores must have shape (B, C, H, W), got {tuple(z.shape)}")
        b, c, h, w = z.shape
        if c != self.classes:
            raise RuntimeError(f"the scores have {c} channels, the extractor {self.classes} classes")
        if h < 1 or w < 1:
            raise RuntimeError(f"scores need H, W >= 1, got {tuple(z.shape)}")
        _check_path_costs(self.qmax, h, w)
        return z.detach().contiguous(), b, h, w

    def _desc(self, images, h, w, t, scores):
        elem = (L.SURF_BF16 if t.dtype == torch.bfloat16 else L.SURF_F32) if scores else _elem(t)
        return L.SurfDesc(images, h, w, self.classes, elem, len(self.order), -1 if self.max_step is None else self.max_step,
                          int(self.ignore_index is not None), len(self.keep), self.qmax, self.scale, 0, int(self.ignore_index or 0))

    # ---- extraction ---------------------------------------------------------------------------------------------------------
    def _extract(self, t, images, h, w, scores, lead):
        _need_device(t)
        k = len(self.order)
        out = torch.empty(tuple(lead) + (k - 1, w), dtype=torch.int32, device=t.device)
        if images == 0:
            return out
        lib = L.lib()
        if self.max_step is None:      # no workspace: only the 2^31 pixels of a call bound a chunk
            chunks = _image_chunks(images, h, w, 1, images)
        else:
            one = int(lib.oct_surf_workspace_bytes(C.byref(self._desc(1, h, w, t, scores))))
            if one == 0:
                raise L.OctError(f"oct_surf_workspace_bytes failed: {L.last_error()}")
            chunks = _image_chunks(images, h, w, one, self.max_workspace_bytes)
        flat = t.reshape((images, self.classes, h, w) if scores else (images, h, w))
        surf = out.reshape(images, k - 1, w)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        for lo, n in chunks:
            desc = self._desc(n, h, w, t, scores)
            ws = None
            if self.max_step is not None:
                need = int(lib.oct_surf_workspace_bytes(C.byref(desc)))
                self._workspace = _grown(self._workspace, need, t.device)
                ws = self._workspace.data_ptr()
            L.check(lib.oct_surf_extract(C.byref(desc), self._order, flat[lo:lo + n].data_ptr(), surf[lo:lo + n].data_ptr(), ws, stream),
                    "oct_surf_extract")
        return out

    def extract(self, map):
        """int32 (*lead, K-1, W): the surfaces of an integer class map (*lead, H, W)"""
        m, images, h, w = self._map(map)
        return self._extract(m, images, h, w, False, m.shape[:-2])

    def extract_scores(self, scores):
        """int32 (B, K-1, W): the surfaces of NCHW fp32 / bf16 scores (B, C, H, W)"""
        z, images, h, w = self._scores(scores)
        return self._extract(z, images, h, w, True, (images,))

    @torch.no_grad()
    def from_model(self, model, x):
        """extract_scores(model.logits(x)) of an engine network (UNet, BioUNet) in its current mode"""
        if not callable(getattr(model, "logits", None)):
            raise TypeError(f"from_model takes a network with logits(x), got {type(model).__name__}")
        return self.extract_scores(model.logits(x))

    # ---- painting -----------------------------------------------------------------------------------------------------------
    def paint(self, map_or_scores, surfaces, out=None):
        """The map the surfaces describe, with the classes of `keep` left where the input has them: the input map's shape and
        dtype, or int64 (B, H, W) for scores (a floating-point tensor is read as scores).  `out` may be a contiguous tensor of
        that shape and dtype to write into -- the converted input map itself to paint in place."""
        t = map_or_scores
        scores = torch.is_tensor(t) and t.is_floating_point()
        if scores:
            t, images, h, w = self._scores(t)
            shape, dtype = (images, h, w), torch.int64
        else:
            t, images, h, w = self._map(t)
            shape, dtype = tuple(t.shape), t.dtype
        surfaces = _check_surfaces(surfaces, images, len(self.order), w, t.device)
        _need_device(t)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=t.device)
        elif not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != dtype or out.device != t.device or \
                not out.is_contiguous():
            raise RuntimeError(f"out must be a contiguous {dtype} tensor of shape {shape} on {t.device}")
        if images == 0:
            return out
        stream = torch.cuda.current_stream(t.device).cuda_stream
        per = max(1, (2 ** 31 - 1) // (h * w))
        flat = t.reshape((images, self.classes, h, w) if scores else (images, h, w))
        surf, dst = surfaces.reshape(images, -1, w), out.reshape(images, h, w)
        for lo in range(0, images, per):
            n = min(per, images - lo)
            L.check(L.lib().oct_surf_paint(C.byref(self._desc(n, h, w, t, scores)), self._order, self._keep, flat[lo:lo + n].data_ptr(),
                                           surf[lo:lo + n].data_ptr(), dst[lo:lo + n].data_ptr(), stream), "oct_surf_paint")
        return out

    def __call__(self, map, out=None):
        """extract followed by paint: the topologically valid version of an integer class map"""
        return self.paint(map, self.extract(map), out)
