"""Paired image / label augmentation on the device (csrc/augment.hip): ONE launch per batch warps the image, the class map,
the multi-label mask and the pixel-weight map with the same per-sample geometry and runs gain / bias / gamma / speckle on the
image.  What comes out feeds forward_backward, loss, forward_backward_binary, DDPTrainer.step and the evaluators unchanged.

Everything is a pure function of (seed, step, global sample index): the parameters are drawn on the host with Philox4x32-10
under the counter (k, 0xFFFFFFFF, global index, step), the pixel noise on the device with the same generator under
((pixel >> 1), channel, global index, step).  Neither the batch split nor the number of ranks changes a sample.

Geometry (include/oct_hip.h has the full statement).  Pixel centres sit at integer coordinates.  Per sample six Q24 integers
a b c / d e f map the output pixel (xo, yo) to the source point SX = a xo + b yo + c, SY = d xo + e yo + f; an optional
elastic displacement (int32 Q24 nodes on a control grid of pitch 2^k, blended bilinearly in integers) is added.  Images and
the weight map are sampled bilinearly (taps outside read `fill` / 0), labels by the nearest pixel (outside reads `label_fill`:
set it to the loss's ignore_index and the warped-in border is ignored).

  AugmentParams    per-sample matrices, intensity parameters and displacements of one batch, built on the host in float64 and
                   quantised once, round-half-even: identity / hflip / vflip / compose / from_matrices
  augment_pair     the launch on explicit parameters
  PairAugmenter    draws the parameters and launches; state_dict() is {seed, step}

Not provided: per-image z-score (it needs a reduction pass), 3-D volumes, capture into a HIP graph (the parameters of every
call come from the host).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

Q = 24
ONE = 1 << Q
MAX_DIM = L.AUG_MAX_DIM
MAX_COEF = 8.0            # |a|, |b|, |d|, |e| stay below this
MAX_OFFSET = 1 << 40      # |c|, |f| (Q24) stay below this: 65536 pixels
MAX_DISP_PX = 64.0
PARAM_CHANNEL = 0xFFFFFFFF   # the "channel" word of the host draws: no image channel reaches it
ELASTIC_K0 = 16              # first counter word 0 of the elastic nodes (below: the scalar draws)

_SRC_ELEM = {torch.uint8: L.AUG_U8, torch.bfloat16: L.AUG_BF16, torch.float32: L.AUG_F32}
_OUT_ELEM = {torch.bfloat16: L.AUG_BF16, torch.float32: L.AUG_F32}
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 on the host: counter (..., 4) and key (2,) of 32-bit words -> uint32 (..., 4).  The generator of
    oct_augment_pair (Salmon et al., SC'11), vectorised over the leading axes."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK32
    if c.shape[-1] != 4:
        raise ValueError(f"counter must end in 4 words, got shape {c.shape}")
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2   # 32 x 32 -> 64 bits: no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _hw(v, what):
    if isinstance(v, int) and not isinstance(v, bool):
        v = (v, v)
    try:
        h, w = (int(s) for s in v)
    except Exception:
        raise TypeError(f"{what} must be an int or (height, width), got {v!r}") from None
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f"{what} {(h, w)} is not accepted by the geometry: sizes are 1..{MAX_DIM}")
    return h, w


def grid_shape(out_hw, pitch):
    """(gh, gw) of the control grid of pitch `pitch` over an output of out_hw: ceil((n - 1) / P) + 1 nodes along each axis"""
    ho, wo = out_hw
    return -(-(ho - 1) // pitch) + 1, -(-(wo - 1) // pitch) + 1


def _check_pitch(pitch):
    if isinstance(pitch, bool) or not isinstance(pitch, int) or pitch < 1 or pitch > 1024 or pitch & (pitch - 1):
        raise ValueError(f"elastic pitch must be a power of two in [1, 1024], got {pitch!r}")
    return pitch


def _per_sample(v, batch, what):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(batch, float(a))
    if a.shape != (batch,):
        raise ValueError(f"{what} must be a scalar or have one entry per sample ({batch}), got shape {a.shape}")
    return a


class AugmentParams:
    """The parameters of one batch, on the host.
        matrix     int64 (B, 6): a b c d e f in Q24
        intensity  float32 (B, 7): gain, bias, gamma, sigma_speckle, sigma_add, out_lo, out_hi
        gamma / noise  whether those stages run at all (a stage that is off is skipped, not run with neutral values)
        disp, pitch    int32 Q24 (B, 2, gh, gw) displacement nodes (plane 0 = x, 1 = y) and their pitch, or None"""

    def __init__(self, matrix, src_hw, out_hw, intensity=None, gamma=False, noise=False, disp=None, pitch=None):
        self.src_hw, self.out_hw = _hw(src_hw, "src_hw"), _hw(out_hw, "out_hw")
        m = np.asarray(matrix)
        if m.dtype.kind not in "iu" or m.ndim != 2 or m.shape[1] != 6:
            raise ValueError(f"matrix must be an integer array of shape (B, 6), got {m.dtype} {m.shape}")
        m = m.astype(np.int64)
        lin, off = m[:, [0, 1, 3, 4]], m[:, [2, 5]]
        if m.size and (np.abs(lin).max() >= MAX_COEF * ONE or np.abs(off).max() >= MAX_OFFSET):
            raise ValueError(f"matrix is not accepted by the geometry: |a|, |b|, |d|, |e| < {MAX_COEF} and |c|, |f| < "
                             f"{MAX_OFFSET >> Q} pixels")
        self.matrix = m
        b = m.shape[0]
        if intensity is None:
            intensity = np.tile(np.array([1, 0, 1, 0, 0, -np.inf, np.inf], dtype=np.float32), (b, 1))
        it = np.asarray(intensity, dtype=np.float32)
        if it.shape != (b, 7):
            raise ValueError(f"intensity must have shape {(b, 7)}, got {it.shape}")
        if np.isnan(it).any() or np.isinf(it[:, :5]).any():
            raise ValueError("intensity parameters must be finite (out_lo / out_hi may be infinite)")
        self.intensity = it.copy()
        self.gamma, self.noise = bool(gamma), bool(noise)
        self.disp, self.pitch = None, None
        if disp is not None:
            self.pitch = _check_pitch(pitch)
            d = np.asarray(disp)
            want = (b, 2) + grid_shape(self.out_hw, self.pitch)
            if d.dtype != np.int32 or d.shape != want:
                raise ValueError(f"disp must be int32 of shape {want} for pitch {self.pitch}, got {d.dtype} {d.shape}")
            if d.size and np.abs(d.astype(np.int64)).max() > int(MAX_DISP_PX * ONE):
                raise ValueError(f"displacements are at most {MAX_DISP_PX:g} pixels")
            self.disp = np.ascontiguousarray(d)

    @property
    def batch(self):
        return self.matrix.shape[0]

    @property
    def flags(self):
        return (L.AUG_GAMMA if self.gamma else 0) | (L.AUG_NOISE if self.noise else 0) | (L.AUG_ELASTIC if self.disp is not None else 0)

    # ---- builders: float64 on the host, quantised once, round-half-even ------------------------------------------------------
    @staticmethod
    def from_matrices(mats, src_hw, out_hw, **kw):
        """mats float64 (B, 2, 3): rows (a b c) and (d e f) in pixels, output pixel -> source point"""
        m = np.asarray(mats, dtype=np.float64)
        if m.ndim != 3 or m.shape[1:] != (2, 3):
            raise ValueError(f"mats must have shape (B, 2, 3), got {m.shape}")
        if not np.isfinite(m).all():
            raise ValueError("mats must be finite")
        if m.size and np.abs(m).max() >= float(MAX_OFFSET >> Q):
            raise ValueError("mats are not accepted by the geometry (an entry of 65536 or more)")
        return AugmentParams(np.rint(m * float(ONE)).astype(np.int64).reshape(-1, 6), src_hw, out_hw, **kw)

    @staticmethod
    def compose(batch, src_hw, out_hw=None, hflip=False, vflip=False, rotate_deg=0.0, scale=1.0, translate=(0.0, 0.0),
                crop_offset=None, **kw):
        """centre -> flip -> rotate -> scale -> translate -> crop offset, each a scalar or one entry per sample.
        The content is flipped about the source centre, rotated by rotate_deg (positive = counter-clockwise on screen), enlarged
        by `scale` (a scalar, or (sy, sx)) and moved by translate = (tx, ty) OUTPUT pixels (positive = right / down); then the
        window of out_hw is cut.  crop_offset = (oy, ox) is the source pixel under output pixel (0, 0) of the unaugmented window;
        None centres the window on the source (a half-pixel position when the sizes differ by an odd number)."""
        hs, ws = _hw(src_hw, "src_hw")
        ho, wo = _hw(out_hw if out_hw is not None else src_hw, "out_hw")
        fx = np.where(_per_sample(np.asarray(hflip, dtype=np.float64), batch, "hflip") != 0, -1.0, 1.0)
        fy = np.where(_per_sample(np.asarray(vflip, dtype=np.float64), batch, "vflip") != 0, -1.0, 1.0)
        th = np.deg2rad(_per_sample(rotate_deg, batch, "rotate_deg"))
        if isinstance(scale, (tuple, list)) and len(scale) == 2:
            sy, sx = _per_sample(scale[0], batch, "scale"), _per_sample(scale[1], batch, "scale")
        else:
            sy = sx = _per_sample(scale, batch, "scale")
        if (sx <= 0).any() or (sy <= 0).any():
            raise ValueError("scale must be positive")
        tx, ty = _per_sample(translate[0], batch, "translate"), _per_sample(translate[1], batch, "translate")
        cxo, cyo = (wo - 1) / 2.0, (ho - 1) / 2.0
        if crop_offset is None:
            cxs, cys = np.full(batch, (ws - 1) / 2.0), np.full(batch, (hs - 1) / 2.0)
        else:
            cys = _per_sample(crop_offset[0], batch, "crop_offset") + cyo
            cxs = _per_sample(crop_offset[1], batch, "crop_offset") + cxo
        cos, sin = np.cos(th), np.sin(th)
        # output -> source: undo the translation, the scale, the rotation and the flip, in that order
        a, b = fx * cos / sx, -fx * sin / sy
        d, e = fy * sin / sx, fy * cos / sy
        c = cxs - a * (cxo + tx) - b * (cyo + ty)
        f = cys - d * (cxo + tx) - e * (cyo + ty)
        mats = np.stack([np.stack([a, b, c], axis=-1), np.stack([d, e, f], axis=-1)], axis=1)
        return AugmentParams.from_matrices(mats, (hs, ws), (ho, wo), **kw)

    @staticmethod
    def identity(batch, src_hw, out_hw=None, **kw):
        """no change; with a smaller (larger) out_hw the centred window (frame), on whole pixels"""
        hs, ws = _hw(src_hw, "src_hw")
        ho, wo = _hw(out_hw if out_hw is not None else src_hw, "out_hw")
        return AugmentParams.compose(batch, (hs, ws), (ho, wo), crop_offset=((hs - ho) // 2, (ws - wo) // 2), **kw)

    @staticmethod
    def hflip(batch, src_hw, out_hw=None, **kw):
        return AugmentParams.compose(batch, src_hw, out_hw, hflip=True, **kw)

    @staticmethod
    def vflip(batch, src_hw, out_hw=None, **kw):
        return AugmentParams.compose(batch, src_hw, out_hw, vflip=True, **kw)

    def with_intensity(self, gain=1.0, bias=0.0, gamma=None, speckle=0.0, noise=0.0, clamp=None):
        """a copy with these intensity parameters (scalars or one entry per sample); gamma=None and speckle == noise == 0 leave
        the stage off"""
        b = self.batch
        it = np.empty((b, 7), dtype=np.float32)
        it[:, 0], it[:, 1] = _per_sample(gain, b, "gain"), _per_sample(bias, b, "bias")
        it[:, 2] = 1.0 if gamma is None else _per_sample(gamma, b, "gamma")
        sp, ad = _per_sample(speckle, b, "speckle"), _per_sample(noise, b, "noise")
        it[:, 3], it[:, 4] = sp, ad
        lo, hi = (-np.inf, np.inf) if clamp is None else clamp
        it[:, 5], it[:, 6] = _per_sample(lo, b, "clamp"), _per_sample(hi, b, "clamp")
        return AugmentParams(self.matrix, self.src_hw, self.out_hw, it, gamma is not None, bool((sp != 0).any() or (ad != 0).any()),
                             self.disp, self.pitch)

    def with_displacement(self, disp, pitch):
        return AugmentParams(self.matrix, self.src_hw, self.out_hw, self.intensity, self.gamma, self.noise, disp, pitch)

    def words(self):
        """uint32 (B, 16): the params buffer of oct_augment_pair"""
        w = np.zeros((self.batch, L.AUG_PARAM_WORDS), dtype=np.uint32)
        m = self.matrix
        w[:, 0:4] = m[:, [0, 1, 3, 4]].astype(np.int32).view(np.uint32)
        w[:, 4:8] = np.ascontiguousarray(m[:, [2, 5]]).view(np.uint32).reshape(-1, 4)   # little endian: low word first
        w[:, 8:15] = self.intensity.view(np.uint32)
        return w


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _need_device(t, what, device=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a torch tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise L.OctError(f"{what} is on {t.device}: the HIP path needs a device tensor (there is no CPU fallback)")
    if device is not None and t.device != device:
        raise RuntimeError(f"{what} is on {t.device}, the image on {device}")


def augment_pair(x, params, target=None, mask=None, pixel_weight=None, out_dtype=torch.bfloat16, fill=0.0, label_fill=0,
                 seed=0, step=0, sample_base=0):
    """One augmentation launch on explicit parameters (an AugmentParams): (x_aug, target_aug | None, mask_aug | None,
    weight_aug | None).  x (B, Cin, Hs, Ws) uint8 / bf16 / fp32; target (B, Hs, Ws) uint8 / int64 -> int64; mask (B, C, Hs, Ws)
    uint8 / bool -> uint8; pixel_weight (B, Hs, Ws) fp32.  With a target AND a mask the mask takes a second launch of the same
    kernel without the image.  The parameters travel in one pinned buffer, copied with non_blocking=True: no synchronisation."""
    _need_device(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"x must be (B, C, H, W), got {tuple(x.shape)}")
    if x.dtype not in _SRC_ELEM:
        raise L.OctError(f"x must be uint8, bf16 or fp32 (got {x.dtype})")
    if out_dtype not in _OUT_ELEM:
        raise L.OctError(f"out_dtype must be torch.bfloat16 or torch.float32 (got {out_dtype})")
    if not isinstance(params, AugmentParams):
        raise TypeError(f"params must be an AugmentParams, got {type(params).__name__}")
    b, cin, hs, ws = x.shape
    if cin < 1:
        raise RuntimeError(f"x needs at least one channel, got {tuple(x.shape)}")
    _hw((hs, ws), "the size of x")
    if params.batch != b or params.src_hw != (hs, ws):
        raise RuntimeError(f"params are for {params.batch} samples of {params.src_hw}, x has {b} of {(hs, ws)}")
    if isinstance(label_fill, bool) or not isinstance(label_fill, int) or not -2 ** 63 <= label_fill < 2 ** 63:
        raise TypeError(f"label_fill must be an int64, got {label_fill!r}")
    if not math.isfinite(float(fill)):
        raise ValueError(f"fill must be finite, got {fill!r}")
    dev = x.device
    ho, wo = params.out_hw
    if target is not None:
        _need_device(target, "target", dev)
        if target.dtype not in (torch.uint8, torch.int64) or tuple(target.shape) != (b, hs, ws):
            raise RuntimeError(f"target must be uint8 or int64 of shape {(b, hs, ws)}, got {target.dtype} {tuple(target.shape)}")
        target = target.contiguous()
    if mask is not None:
        _need_device(mask, "mask", dev)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype != torch.uint8 or mask.dim() != 4 or mask.shape[0] != b or tuple(mask.shape[2:]) != (hs, ws) or mask.shape[1] < 1:
            raise RuntimeError(f"mask must be uint8 of shape {(b, 'C', hs, ws)}, got {mask.dtype} {tuple(mask.shape)}")
        if not 0 <= label_fill <= 255:
            raise ValueError(f"label_fill {label_fill} does not fit the uint8 mask")
        mask = mask.contiguous()
    if pixel_weight is not None:
        _need_device(pixel_weight, "pixel_weight", dev)
        if pixel_weight.dtype != torch.float32 or tuple(pixel_weight.shape) != (b, hs, ws):
            raise RuntimeError(f"pixel_weight must be fp32 of shape {(b, hs, ws)}, got {pixel_weight.dtype} {tuple(pixel_weight.shape)}")
        pixel_weight = pixel_weight.detach().contiguous()
    x = x.detach().contiguous()

    x_out = torch.empty((b, cin, ho, wo), dtype=out_dtype, device=dev)
    t_out = torch.empty((b, ho, wo), dtype=torch.int64, device=dev) if target is not None else None
    m_out = torch.empty((b, mask.shape[1], ho, wo), dtype=torch.uint8, device=dev) if mask is not None else None
    w_out = torch.empty((b, ho, wo), dtype=torch.float32, device=dev) if pixel_weight is not None else None
    if b == 0:
        return x_out, t_out, m_out, w_out

    # one pinned buffer: [B][16] parameter words, then the displacement nodes.  The caching host allocator keeps the block
    # alive until the copy has run, so the call returns without waiting for it.
    words = params.words()
    ndisp = params.disp.size if params.disp is not None else 0
    host = torch.empty(words.size + ndisp, dtype=torch.int32, pin_memory=True)
    hv = host.numpy()
    hv[:words.size] = words.reshape(-1).view(np.int32)
    if ndisp:
        hv[words.size:] = params.disp.reshape(-1)
    buf = host.to(dev, non_blocking=True)
    disp_ptr = buf.data_ptr() + 4 * words.size if ndisp else None

    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lib, st = L.lib(), _stream(dev)

    def desc(cin_, kind, planes):
        return L.AugmentDesc(b, cin_, hs, ws, ho, wo, _SRC_ELEM[x.dtype], _OUT_ELEM[out_dtype], kind, planes, params.flags,
                             params.pitch or 0, seed & 0xFFFFFFFF, seed >> 32, int(step) & 0xFFFFFFFF,
                             int(sample_base) & 0xFFFFFFFF, float(fill), 0, label_fill)

    if target is not None:
        kind, lab, lab_out, planes = (L.AUG_LABEL_CLASS_U8 if target.dtype == torch.uint8 else L.AUG_LABEL_CLASS_I64), target, t_out, 1
    elif mask is not None:
        kind, lab, lab_out, planes = L.AUG_LABEL_MASK_U8, mask, m_out, mask.shape[1]
    else:
        kind, lab, lab_out, planes = L.AUG_LABEL_NONE, None, None, 0
    d = desc(cin, kind, planes)
    L.check(lib.oct_augment_pair(C.byref(d), x.data_ptr(), L.ptr(lab), L.ptr(pixel_weight), buf.data_ptr(), disp_ptr,
                                 x_out.data_ptr(), L.ptr(lab_out), L.ptr(w_out), st), "oct_augment_pair")
    if target is not None and mask is not None:
        d = desc(0, L.AUG_LABEL_MASK_U8, mask.shape[1])
        L.check(lib.oct_augment_pair(C.byref(d), None, mask.data_ptr(), None, buf.data_ptr(), disp_ptr, None, m_out.data_ptr(),
                                     None, st), "oct_augment_pair")
    return x_out, t_out, m_out, w_out


def philox_words_device(counters, key):
    """raw Philox words from the device generator: counters uint32-valued int64 / int32 tensor (n, 4) on the device ->
    int64 tensor (n, 4) of words.  Exists so that the generator can be pinned bit for bit."""
    _need_device(counters, "counters")
    if counters.dim() != 2 or counters.shape[1] != 4:
        raise RuntimeError(f"counters must have shape (n, 4), got {tuple(counters.shape)}")
    c32 = (counters.to(torch.int64) & 0xFFFFFFFF).to(torch.int32).contiguous()   # wraps into the 32 bits of the word
    out = torch.empty_like(c32)
    L.check(L.lib().oct_augment_philox_words(c32.data_ptr(), c32.shape[0], int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF,
                                             out.data_ptr(), _stream(counters.device)), "oct_augment_philox_words")
    return out.to(torch.int64) & 0xFFFFFFFF


def _range(v, what, lo_ok=None):
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = (v, v)
    try:
        lo, hi = (float(s) for s in v)
    except Exception:
        raise TypeError(f"{what} must be a number or (low, high), got {v!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"{what} must be a finite (low, high) with low <= high, got {(lo, hi)}")
    if lo_ok is not None and lo <= lo_ok:
        raise ValueError(f"{what} must stay above {lo_ok}, got {(lo, hi)}")
    return lo, hi


class PairAugmenter:
    """Draws the augmentation of every sample and applies it in one launch:

        aug = PairAugmenter(hflip=0.5, rotate_deg=10, scale=(0.9, 1.1), translate=(0.0, 0.05), elastic_pitch=32,
                            elastic_sigma_px=4, gain=(0.9, 1.1), gamma=(0.8, 1.25), speckle=0.1, label_fill=255, seed=1, rank=r)
        x, t, _, w = aug(x_u8, target=t_u8, pixel_weight=w_map)
        model.forward_backward(x, t, 1.0, 0.5, pixel_weight=w, ignore_index=255)

    hflip / vflip are probabilities; rotate_deg r draws an angle in [-r, r]; scale, gain, bias, gamma are (low, high) ranges
    (gamma=None leaves the stage off); translate = (fx, fy) draws a shift within +-fx * width, +-fy * height; the elastic nodes
    are N(0, elastic_sigma_px) pixels, cut at 3 sigma (at most 64); speckle / noise are the sigmas of the multiplicative / additive
    noise; clamp = (low, high) bounds the output.  out_size cuts a centred window (on whole pixels) of that size; `scale` zooms
    within it.  Sample b of a call has global index rank * B + b; step advances once per call."""

    def __init__(self, out_size=None, hflip=0.0, vflip=0.0, rotate_deg=0.0, scale=(1, 1), translate=(0.0, 0.0), elastic_pitch=None,
                 elastic_sigma_px=0.0, gain=(1, 1), bias=(0, 0), gamma=None, speckle=0.0, noise=0.0, clamp=None, fill=0.0,
                 label_fill=0, out_dtype=torch.bfloat16, seed=0, rank=0):
        self.out_size = None if out_size is None else _hw(out_size, "out_size")
        for name, p in (("hflip", hflip), ("vflip", vflip)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"{name} is a probability in [0, 1], got {p!r}")
        self.hflip, self.vflip = float(hflip), float(vflip)
        self.rotate_deg = float(rotate_deg)
        if not 0.0 <= self.rotate_deg <= 180.0:
            raise ValueError(f"rotate_deg must be in [0, 180], got {rotate_deg!r}")
        self.scale = _range(scale, "scale", lo_ok=0.0)
        if self.scale[0] < 0.25 or self.scale[1] > 4.0:
            raise ValueError(f"scale must stay within [0.25, 4], got {self.scale}")
        try:
            self.translate = (float(translate[0]), float(translate[1]))
        except Exception:
            raise TypeError(f"translate must be (fraction of width, fraction of height), got {translate!r}") from None
        if min(self.translate) < 0 or max(self.translate) > 1:
            raise ValueError(f"translate fractions must be in [0, 1], got {self.translate}")
        self.elastic_pitch = None if elastic_pitch is None else _check_pitch(elastic_pitch)
        self.elastic_sigma_px = float(elastic_sigma_px)
        if self.elastic_sigma_px < 0 or not math.isfinite(self.elastic_sigma_px):
            raise ValueError(f"elastic_sigma_px must be >= 0, got {elastic_sigma_px!r}")
        if self.elastic_sigma_px > 0 and self.elastic_pitch is None:
            raise ValueError("elastic_sigma_px needs elastic_pitch")
        self.gain, self.bias = _range(gain, "gain"), _range(bias, "bias")
        self.gamma = None if gamma is None else _range(gamma, "gamma", lo_ok=0.0)
        self.speckle, self.noise = float(speckle), float(noise)
        if self.speckle < 0 or self.noise < 0 or not math.isfinite(self.speckle + self.noise):
            raise ValueError(f"speckle and noise are sigmas >= 0, got {speckle!r}, {noise!r}")
        self.clamp = None if clamp is None else tuple(float(v) for v in clamp)
        if self.clamp is not None and (len(self.clamp) != 2 or not self.clamp[0] <= self.clamp[1]):
            raise ValueError(f"clamp must be (low, high) with low <= high, got {clamp!r}")
        if not math.isfinite(float(fill)):
            raise ValueError(f"fill must be finite, got {fill!r}")
        self.fill = float(fill)
        if isinstance(label_fill, bool) or not isinstance(label_fill, int) or not -2 ** 63 <= label_fill < 2 ** 63:
            raise TypeError(f"label_fill must be an int64, got {label_fill!r}")
        self.label_fill = label_fill
        if out_dtype not in _OUT_ELEM:
            raise L.OctError(f"out_dtype must be torch.bfloat16 or torch.float32 (got {out_dtype})")
        self.out_dtype = out_dtype
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise TypeError(f"seed must be an int in [0, 2^64), got {seed!r}")
        if isinstance(rank, bool) or not isinstance(rank, int) or rank < 0:
            raise TypeError(f"rank must be an int >= 0, got {rank!r}")
        self.seed, self.rank, self.step = seed, rank, 0

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state):
        seed, step = state["seed"], state["step"]
        if not (isinstance(seed, int) and 0 <= seed < 2 ** 64 and isinstance(step, int) and 0 <= step < 2 ** 32):
            raise ValueError(f"bad augmenter state {state!r}")
        self.seed, self.step = seed, step

    def _key(self):
        return self.seed & 0xFFFFFFFF, self.seed >> 32

    def draw(self, batch, src_hw, step=None, sample_base=None):
        """the AugmentParams of samples sample_base .. sample_base + batch - 1 (default rank * batch) at `step` (default the
        augmenter's): a function of (seed, step, global index) and the sizes alone"""
        hs, ws = _hw(src_hw, "src_hw")
        ho, wo = self.out_size or (hs, ws)
        step = self.step if step is None else int(step)
        base = self.rank * batch if sample_base is None else int(sample_base)
        gidx = (base + np.arange(batch, dtype=np.uint64)) & _MASK32
        ctr = np.empty((batch, 3, 4), dtype=np.uint64)
        ctr[:, :, 0] = np.arange(3, dtype=np.uint64)[None, :]
        ctr[:, :, 1] = PARAM_CHANNEL
        ctr[:, :, 2] = gidx[:, None]
        ctr[:, :, 3] = step & 0xFFFFFFFF
        u = ((philox4x32_10(ctr, self._key()).astype(np.float64) + 0.5) * 2.0 ** -32).reshape(batch, 12)   # (0, 1)

        def span(col, lo, hi):
            return lo + (hi - lo) * u[:, col]

        p = AugmentParams.compose(
            batch, (hs, ws), (ho, wo), hflip=u[:, 0] < self.hflip, vflip=u[:, 1] < self.vflip,
            rotate_deg=span(2, -self.rotate_deg, self.rotate_deg), scale=span(3, *self.scale),
            translate=(span(4, -self.translate[0], self.translate[0]) * wo, span(5, -self.translate[1], self.translate[1]) * ho),
            crop_offset=((hs - ho) // 2, (ws - wo) // 2))
        p = p.with_intensity(gain=span(6, *self.gain), bias=span(7, *self.bias),
                             gamma=None if self.gamma is None else span(8, *self.gamma),
                             speckle=self.speckle, noise=self.noise, clamp=self.clamp)
        if self.elastic_pitch is not None and self.elastic_sigma_px > 0:
            gh, gw = grid_shape((ho, wo), self.elastic_pitch)
            nc = np.empty((batch, gh * gw, 4), dtype=np.uint64)
            nc[:, :, 0] = (ELASTIC_K0 + np.arange(gh * gw, dtype=np.uint64))[None, :]
            nc[:, :, 1] = PARAM_CHANNEL
            nc[:, :, 2] = gidx[:, None]
            nc[:, :, 3] = step & 0xFFFFFFFF
            w = philox4x32_10(nc, self._key()).astype(np.float64)
            r = np.sqrt(-2.0 * np.log((w[..., 0] + 0.5) * 2.0 ** -32))
            ang = 2.0 * np.pi * w[..., 1] * 2.0 ** -32
            cut = min(3.0 * self.elastic_sigma_px, MAX_DISP_PX)
            dx = np.clip(self.elastic_sigma_px * r * np.cos(ang), -cut, cut)
            dy = np.clip(self.elastic_sigma_px * r * np.sin(ang), -cut, cut)
            disp = np.rint(np.stack([dx, dy], axis=1) * float(ONE)).astype(np.int32).reshape(batch, 2, gh, gw)
            p = p.with_displacement(disp, self.elastic_pitch)
        return p

    def __call__(self, x, target=None, mask=None, pixel_weight=None, params=None):
        _need_device(x, "x")
        if x.dim() != 4:
            raise RuntimeError(f"x must be (B, C, H, W), got {tuple(x.shape)}")
        b, _, hs, ws = x.shape
        if params is None:
            params = self.draw(b, (hs, ws))
        elif not isinstance(params, AugmentParams):
            raise TypeError(f"params must be an AugmentParams, got {type(params).__name__}")
        elif self.out_size is not None and params.out_hw != self.out_size:
            raise RuntimeError(f"params are for an output of {params.out_hw}, the augmenter's out_size is {self.out_size}")
        out = augment_pair(x, params, target, mask, pixel_weight, self.out_dtype, self.fill, self.label_fill, self.seed, self.step,
                           self.rank * b)
        self.step = (self.step + 1) & 0xFFFFFFFF
        return out
