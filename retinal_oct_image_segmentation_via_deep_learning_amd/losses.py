"""Cross-entropy + soft-Dice loss on network logits (csrc/seg_loss.hip), and the training extras of the logits networks.

The loss is the fused UNet head's (oracle/ref_cpu.py::loss_head_fwd / loss_head_bwd): CE = mean over pixels of
-log softmax[target], Dice = 1 - mean_c (2 I_c + eps) / (P_c + Y_c + eps), loss = w_ce CE + w_dice Dice.  The per-workgroup
rows of the loss kernels are reduced by oct_head_loss_finalize, so both heads share one definition.

With class_weight / pixel_weight / ignore_index (each optional; the oct_seg_loss_*_weighted kernels):
  omega_i = [t_i != ignore_index] * class_weight[t_i] * pixel_weight[i],   CE = sum omega_i ce_i / sum omega_i
(F.cross_entropy(weight=, ignore_index=) when there is no map), and the Dice sums run over the pixels that are not ignored.
sum omega is reduced on the device and read there by the backward kernel: a weighted step synchronises as little as an
unweighted one, and a CE-only step still reads the logits once.  With all three absent the unweighted kernels run, unchanged.

  cross_entropy_dice(logits, target, ...)  NCHW fp32 logits (any network's output) -> 0-d differentiable loss; with
                                           w_dice == 0 a drop-in for F.cross_entropy(logits, target)
  SegLossMixin                             forward_backward / loss / predict for the networks that return logits
                                           (U_Net, AttU_Net, AttU_Net4, MGUNet, MGUNet_2, ReLayNet), on the NHWC logits the
                                           network writes: no NCHW copy, no ATen softmax / NLL

Binary / multi-label head (the oct_bce_loss_* kernels): C independent sigmoid channels against a uint8 mask (B, C, H, W).
  valid = t != ignore_value,  omega = valid * pixel_weight[pixel],  l = BCEWithLogits(x, t, pos_weight[c])
  BCE = sum omega l / sum omega over all B C H W elements,  Dice as above with p = sigmoid(x) over the valid elements
  binary_cross_entropy_dice(logits, target, ...)  with w_dice == 0 a drop-in for F.binary_cross_entropy_with_logits
  SegLossMixin.forward_backward_binary / loss_binary / predict_mask   the same three contracts on the sigmoid head
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import ops
from .engine import _stream

_DT = {torch.bfloat16: L.DT_BF16, torch.float32: L.DT_F32}


def _check_classes(classes: int):
    if classes > L.MAX_CLASSES:
        raise NotImplementedError(f"the HIP loss kernels take at most {L.MAX_CLASSES} classes (got {classes})")


def _geometry(logits, layout):
    """(n, h, w, classes) of an NHWC or NCHW logits tensor, after the checks the kernels rely on."""
    ops._need_cuda(logits)
    if logits.dim() != 4:
        raise RuntimeError(f"expected 4-D logits, got {tuple(logits.shape)}")
    if layout == L.SEG_NCHW:
        if logits.dtype != torch.float32:
            raise L.OctError(f"NCHW logits must be fp32 (got {logits.dtype})")
        n, c, h, w = logits.shape
    else:
        if logits.dtype not in _DT:
            raise L.OctError(f"NHWC logits must be bf16 or fp32 (got {logits.dtype})")
        n, h, w, c = logits.shape
    _check_classes(c)
    return n, h, w, c


def _target(target, n, h, w, device):
    if target.dtype != torch.int64 or tuple(target.shape) != (n, h, w):
        raise RuntimeError(f"target must be int64 of shape {(n, h, w)}, got {target.dtype} {tuple(target.shape)}")
    if target.device != device:
        raise RuntimeError(f"target is on {target.device}, logits on {device}")
    return target.contiguous()


def _options(class_weight, pixel_weight, ignore_index, n, h, w, classes, device):
    """The three options of the weighted loss, checked against the logits' geometry before anything is launched: None when
    all are absent (the unweighted kernels then run), else (class_weight | None, pixel_weight | None, has_ignore, ignore_index)
    with the weights as contiguous fp32 tensors on `device`.  A sequence of floats is converted here, once per call: pass a
    device tensor to convert it once per training run."""
    if class_weight is None and pixel_weight is None and ignore_index is None:
        return None
    device = torch.device(device)
    if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)):
        raise TypeError(f"ignore_index must be an int or None, got {type(ignore_index).__name__} {ignore_index!r}")
    if ignore_index is not None and not -2 ** 63 <= ignore_index < 2 ** 63:
        raise ValueError(f"ignore_index {ignore_index} is not an int64")
    if class_weight is not None:
        if not torch.is_tensor(class_weight):
            vals = [float(v) for v in class_weight]
            if len(vals) != classes:
                raise RuntimeError(f"class_weight must have {classes} entries (one per class), got {len(vals)}")
            class_weight = torch.tensor(vals, dtype=torch.float32, device=device)
        if class_weight.dtype != torch.float32:
            raise RuntimeError(f"class_weight must be fp32, got {class_weight.dtype}")
        if tuple(class_weight.shape) != (classes,):
            raise RuntimeError(f"class_weight must have {classes} entries (one per class), got shape {tuple(class_weight.shape)}")
        if class_weight.device != device:
            raise RuntimeError(f"class_weight is on {class_weight.device}, logits on {device}")
        class_weight = class_weight.detach().contiguous()
    if pixel_weight is not None:
        if not torch.is_tensor(pixel_weight) or pixel_weight.dtype != torch.float32:
            raise RuntimeError(f"pixel_weight must be an fp32 tensor, got {getattr(pixel_weight, 'dtype', type(pixel_weight).__name__)}")
        if tuple(pixel_weight.shape) != (n, h, w):
            raise RuntimeError(f"pixel_weight must have shape {(n, h, w)}, got {tuple(pixel_weight.shape)}")
        if pixel_weight.device != device:
            raise RuntimeError(f"pixel_weight is on {pixel_weight.device}, logits on {device}")
        pixel_weight = pixel_weight.detach().contiguous()
    return class_weight, pixel_weight, int(ignore_index is not None), int(ignore_index or 0)


class _Loss:
    """One launch plan: descriptor, partial rows, [loss, ce, dice] and the Dice backward coefficients."""

    def __init__(self, logits, layout):
        self.layout = layout
        self.n, self.h, self.w, self.c = _geometry(logits, layout)
        self.logits = logits.contiguous()
        self.desc = L.HeadDesc(_DT[logits.dtype], self.n, self.h, self.w, 1, self.c)
        self.blocks = L.lib().oct_seg_loss_blocks(self.n * self.h * self.w, self.c)
        self.dev = logits.device

    def partials(self):
        return torch.empty((self.blocks, L.HEAD_LOSS_SLOTS), dtype=torch.float64, device=self.dev)

    def forward(self, target=None, want_argmax=False):
        """(loss partial rows or None, argmax map or None)"""
        part = self.partials() if target is not None else None
        amax = torch.empty((self.n, self.h, self.w), dtype=torch.int64, device=self.dev) if want_argmax else None
        L.check(L.lib().oct_seg_loss_forward(C.byref(self.desc), self.layout, self.logits.data_ptr(), L.ptr(target),
                                             L.ptr(amax), L.ptr(part), _stream()), "oct_seg_loss_forward")
        return part, amax

    def finalize(self, part, w_ce, w_dice, dice_eps):
        """[loss, ce, dice] (fp32, device) and dice_coef [2][MAX_CLASSES]"""
        out = torch.empty(3, dtype=torch.float32, device=self.dev)
        coef = torch.empty(2 * L.MAX_CLASSES, dtype=torch.float32, device=self.dev)
        L.check(L.lib().oct_head_loss_finalize(C.byref(self.desc), part.data_ptr(), self.blocks, float(w_ce), float(w_dice),
                                               float(dice_eps), out.data_ptr(), coef.data_ptr(), _stream()),
                "oct_head_loss_finalize")
        return out, coef

    def backward(self, target, dice_coef, w_ce, dloss=None, part=None):
        """d(loss)/d(logits) in the logits' layout and dtype; part: CE rows written by the same pass (no Dice term only)"""
        dl = torch.empty_like(self.logits)
        L.check(L.lib().oct_seg_loss_backward(C.byref(self.desc), self.layout, self.logits.data_ptr(), target.data_ptr(),
                                              L.ptr(dice_coef), float(w_ce), L.ptr(dloss), dl.data_ptr(), L.ptr(part),
                                              _stream()), "oct_seg_loss_backward")
        return dl

    # ---- weighted forms: opt = _options(...) ------------------------------------------------------------------------------
    def weight_sum(self, target, opt):
        """sum omega as one device double, from the labels and the map alone"""
        scratch = torch.empty(self.blocks + 1, dtype=torch.float64, device=self.dev)
        cw, pw, has_ig, ig = opt
        L.check(L.lib().oct_seg_loss_weight_sum(C.byref(self.desc), target.data_ptr(), L.ptr(cw), L.ptr(pw), has_ig, ig,
                                                scratch.data_ptr(), scratch[self.blocks:].data_ptr(), _stream()),
                "oct_seg_loss_weight_sum")
        return scratch[self.blocks:]

    def forward_weighted(self, target, opt):
        part = self.partials()
        cw, pw, has_ig, ig = opt
        L.check(L.lib().oct_seg_loss_forward_weighted(C.byref(self.desc), self.layout, self.logits.data_ptr(), target.data_ptr(),
                                                      L.ptr(cw), L.ptr(pw), has_ig, ig, part.data_ptr(), _stream()),
                "oct_seg_loss_forward_weighted")
        return part

    def finalize_weighted(self, part, w_ce, w_dice, dice_eps):
        """[loss, ce, dice], dice_coef and sum omega (device double) of weighted rows"""
        out = torch.empty(3, dtype=torch.float32, device=self.dev)
        coef = torch.empty(2 * L.MAX_CLASSES, dtype=torch.float32, device=self.dev)
        wsum = torch.empty(1, dtype=torch.float64, device=self.dev)
        L.check(L.lib().oct_seg_loss_finalize_weighted(C.byref(self.desc), part.data_ptr(), self.blocks, float(w_ce),
                                                       float(w_dice), float(dice_eps), out.data_ptr(), coef.data_ptr(),
                                                       wsum.data_ptr(), _stream()), "oct_seg_loss_finalize_weighted")
        return out, coef, wsum

    def backward_weighted(self, target, opt, wsum, dice_coef, w_ce, dloss=None, part=None):
        dl = torch.empty_like(self.logits)
        cw, pw, has_ig, ig = opt
        L.check(L.lib().oct_seg_loss_backward_weighted(C.byref(self.desc), self.layout, self.logits.data_ptr(), target.data_ptr(),
                                                       L.ptr(cw), L.ptr(pw), has_ig, ig, wsum.data_ptr(), L.ptr(dice_coef),
                                                       float(w_ce), L.ptr(dloss), dl.data_ptr(), L.ptr(part), _stream()),
                "oct_seg_loss_backward_weighted")
        return dl


def loss_and_dlogits(logits, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7, class_weight=None, pixel_weight=None,
                     ignore_index=None, layout=L.SEG_NHWC):
    """Training head on NHWC logits (or NCHW fp32 ones with layout=SEG_NCHW): ([loss, ce, dice], dlogits).  Without a Dice
    term the backward pass also writes the CE rows (the logits are read once; the Dice entry is then 0); with one, forward
    rows -> finalize -> backward.  With class_weight / pixel_weight / ignore_index the same two schedules on the weighted
    kernels: sum omega comes from a pass over the labels and the map (CE only) or out of the forward rows (with Dice)."""
    h = _Loss(logits, layout)
    t = _target(target, h.n, h.h, h.w, h.dev)
    opt = _options(class_weight, pixel_weight, ignore_index, h.n, h.h, h.w, h.c, h.dev)
    if opt is not None:
        if w_dice == 0.0:
            wsum = h.weight_sum(t, opt)
            part = h.partials()
            dl = h.backward_weighted(t, opt, wsum, None, w_ce, part=part)
            return h.finalize_weighted(part, w_ce, w_dice, dice_eps)[0], dl
        part = h.forward_weighted(t, opt)
        out, coef, wsum = h.finalize_weighted(part, w_ce, w_dice, dice_eps)
        return out, h.backward_weighted(t, opt, wsum, coef, w_ce)
    if w_dice == 0.0:
        part = h.partials()
        dl = h.backward(t, None, w_ce, part=part)
        out, _ = h.finalize(part, w_ce, w_dice, dice_eps)
        return out, dl
    part, _ = h.forward(t)
    out, coef = h.finalize(part, w_ce, w_dice, dice_eps)
    return out, h.backward(t, coef, w_ce)


class _CrossEntropyDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, layout, w_ce, w_dice, dice_eps, class_weight, pixel_weight, ignore_index):
        h = _Loss(logits.detach(), layout)
        t = _target(target, h.n, h.h, h.w, h.dev)
        ctx.opt = _options(class_weight, pixel_weight, ignore_index, h.n, h.h, h.w, h.c, h.dev)
        ctx.wsum = None
        if ctx.opt is not None:
            out, coef, ctx.wsum = h.finalize_weighted(h.forward_weighted(t, ctx.opt), w_ce, w_dice, dice_eps)
        else:
            part, _ = h.forward(t)
            out, coef = h.finalize(part, w_ce, w_dice, dice_eps)
        ctx.h, ctx.t, ctx.w_ce = h, t, w_ce
        ctx.coef = coef if w_dice != 0.0 else None
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        # the upstream gradient stays on the device: the kernel reads it, nothing synchronises
        g = dout.detach().to(torch.float32).contiguous()
        if ctx.opt is not None:
            dl = ctx.h.backward_weighted(ctx.t, ctx.opt, ctx.wsum, ctx.coef, ctx.w_ce, dloss=g)
        else:
            dl = ctx.h.backward(ctx.t, ctx.coef, ctx.w_ce, dloss=g)
        ctx.h = ctx.t = ctx.coef = ctx.opt = ctx.wsum = None
        return dl, None, None, None, None, None, None, None, None


def cross_entropy_dice(logits, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7, class_weight=None, pixel_weight=None,
                       ignore_index=None):
    """w_ce * CE + w_dice * soft Dice of NCHW fp32 CUDA logits (B, C, H, W) against int64 labels (B, H, W): a 0-d loss
    that autograd differentiates through the HIP backward kernel.  w_dice == 0: F.cross_entropy(logits, target).
    A label outside [0, C) gives a NaN loss (torch raises there); at most 16 classes.

    class_weight: fp32 device tensor of C entries (or a sequence of floats, converted on every call); pixel_weight: fp32
    device tensor (B, H, W), a constant of the loss -- no gradient is returned for it; ignore_index: int or None.  With
    class_weight and ignore_index this is F.cross_entropy(logits, target, weight=class_weight, ignore_index=ignore_index);
    a map multiplies each pixel's term and its share of the denominator.  ignore_index defaults to None, not torch's
    -100: a label of -100 keeps giving NaN unless it is named here.  Everything ignored: NaN, as torch."""
    return _CrossEntropyDice.apply(logits, target, L.SEG_NCHW, float(w_ce), float(w_dice), float(dice_eps), class_weight,
                                   pixel_weight, ignore_index)


def loss_only(h, target, w_ce, w_dice, dice_eps, opt):
    """[loss, ce, dice] of a _Loss plan without a backward pass; opt: _options(...) or None"""
    t = _target(target, h.n, h.h, h.w, h.dev)
    if opt is not None:
        return h.finalize_weighted(h.forward_weighted(t, opt), w_ce, w_dice, dice_eps)[0]
    part, _ = h.forward(t)
    return h.finalize(part, w_ce, w_dice, dice_eps)[0]


# ---- binary / multi-label head: sigmoid BCE + soft Dice (oct_bce_loss_*) ---------------------------------------------------
def _binary_target(target, n, c, h, w, device):
    """uint8 view of a uint8 / bool mask of the logits' shape (B, C, H, W); (B, H, W) is accepted for one channel"""
    shapes = ((n, c, h, w), (n, h, w)) if c == 1 else ((n, c, h, w),)
    if not torch.is_tensor(target) or target.dtype not in (torch.uint8, torch.bool) or tuple(target.shape) not in shapes:
        raise RuntimeError(f"target must be uint8 or bool of shape {(n, c, h, w)}, got "
                           f"{getattr(target, 'dtype', type(target).__name__)} {tuple(getattr(target, 'shape', ()))}")
    if target.device != torch.device(device):
        raise RuntimeError(f"target is on {target.device}, logits on {device}")
    t = target.detach().contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _binary_options(pos_weight, pixel_weight, ignore_value, n, h, w, classes, device):
    """The three options of the binary loss, checked against the logits' geometry before anything is launched: None when
    all are absent, else (pos_weight | None, pixel_weight | None, has_ignore, ignore_value) with the weights as contiguous
    fp32 tensors on `device`.  A sequence of floats is converted here, once per call."""
    if pos_weight is None and pixel_weight is None and ignore_value is None:
        return None
    device = torch.device(device)
    if ignore_value is not None and (isinstance(ignore_value, bool) or not isinstance(ignore_value, int)):
        raise TypeError(f"ignore_value must be an int or None, got {type(ignore_value).__name__} {ignore_value!r}")
    if ignore_value is not None and not 2 <= ignore_value <= 255:
        raise ValueError(f"ignore_value {ignore_value} is not in [2, 255] (0 and 1 are the mask's own values)")
    if pos_weight is not None:
        if not torch.is_tensor(pos_weight):
            vals = [float(v) for v in pos_weight]
            if len(vals) != classes:
                raise RuntimeError(f"pos_weight must have {classes} entries (one per channel), got {len(vals)}")
            pos_weight = torch.tensor(vals, dtype=torch.float32, device=device)
        if pos_weight.dtype != torch.float32:
            raise RuntimeError(f"pos_weight must be fp32, got {pos_weight.dtype}")
        if tuple(pos_weight.shape) != (classes,):
            raise RuntimeError(f"pos_weight must have {classes} entries (one per channel), got shape {tuple(pos_weight.shape)}")
        if pos_weight.device != device:
            raise RuntimeError(f"pos_weight is on {pos_weight.device}, logits on {device}")
        pos_weight = pos_weight.detach().contiguous()
    if pixel_weight is not None:
        if not torch.is_tensor(pixel_weight) or pixel_weight.dtype != torch.float32:
            raise RuntimeError(f"pixel_weight must be an fp32 tensor, got {getattr(pixel_weight, 'dtype', type(pixel_weight).__name__)}")
        if tuple(pixel_weight.shape) != (n, h, w):
            raise RuntimeError(f"pixel_weight must have shape {(n, h, w)}, got {tuple(pixel_weight.shape)}")
        if pixel_weight.device != device:
            raise RuntimeError(f"pixel_weight is on {pixel_weight.device}, logits on {device}")
        pixel_weight = pixel_weight.detach().contiguous()
    return pos_weight, pixel_weight, int(ignore_value is not None), int(ignore_value or 0)


def mask_threshold(threshold) -> float:
    """tau = float32(log(threshold / (1 - threshold))): sigmoid(x) >= threshold is x >= tau; 0 at 0.5"""
    import math
    import struct
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 < threshold < 1.0:
        raise ValueError(f"threshold must lie in (0, 1), got {threshold!r}")
    return struct.unpack("f", struct.pack("f", math.log(threshold / (1.0 - threshold))))[0]


class _BinaryLoss(_Loss):
    """The launch plan of _Loss on the sigmoid head; opt: _binary_options(...) or None.  The rows have the weighted CE
    rows' layout, so finalize_weighted reduces them."""

    @staticmethod
    def _opt(opt):
        return opt if opt is not None else (None, None, 0, 0)

    @staticmethod
    def needs_wsum(opt):
        """sum omega is the element count unless a map or ignore_value is there"""
        return opt is not None and (opt[1] is not None or opt[2] != 0)

    def binary_weight_sum(self, target, opt):
        scratch = torch.empty(self.blocks + 1, dtype=torch.float64, device=self.dev)
        _, pm, has_ig, ig = opt
        L.check(L.lib().oct_bce_loss_weight_sum(C.byref(self.desc), target.data_ptr(), L.ptr(pm), has_ig, ig, scratch.data_ptr(),
                                                scratch[self.blocks:].data_ptr(), _stream()), "oct_bce_loss_weight_sum")
        return scratch[self.blocks:]

    def binary_forward(self, target, opt, want_dice):
        part = self.partials()
        pw, pm, has_ig, ig = self._opt(opt)
        L.check(L.lib().oct_bce_loss_forward(C.byref(self.desc), self.layout, self.logits.data_ptr(), target.data_ptr(), L.ptr(pw),
                                             L.ptr(pm), has_ig, ig, int(want_dice), 0.0, None, part.data_ptr(), _stream()),
                "oct_bce_loss_forward")
        return part

    def binary_mask(self, tau):
        """uint8 (B, C, H, W) = logits >= tau"""
        mask = torch.empty((self.n, self.c, self.h, self.w), dtype=torch.uint8, device=self.dev)
        L.check(L.lib().oct_bce_loss_forward(C.byref(self.desc), self.layout, self.logits.data_ptr(), None, None, None, 0, 0, 0,
                                             float(tau), mask.data_ptr(), None, _stream()), "oct_bce_loss_forward")
        return mask

    def binary_backward(self, target, opt, wsum, dice_coef, w_bce, dloss=None, part=None):
        dl = torch.empty_like(self.logits)
        pw, pm, has_ig, ig = self._opt(opt)
        L.check(L.lib().oct_bce_loss_backward(C.byref(self.desc), self.layout, self.logits.data_ptr(), target.data_ptr(), L.ptr(pw),
                                              L.ptr(pm), has_ig, ig, L.ptr(wsum), L.ptr(dice_coef), float(w_bce), L.ptr(dloss),
                                              dl.data_ptr(), L.ptr(part), _stream()), "oct_bce_loss_backward")
        return dl


def binary_loss_and_dlogits(logits, target, w_bce=1.0, w_dice=0.0, dice_eps=1e-7, pos_weight=None, pixel_weight=None,
                            ignore_value=None, layout=L.SEG_NHWC):
    """Training head on NHWC logits (or NCHW fp32 ones with layout=SEG_NCHW): ([loss, bce, dice], dlogits).  Without a Dice
    term the backward pass also writes the BCE rows (the logits are read once; the Dice entry is then 0), after a pass over
    the targets and the map for sum omega when a map or ignore_value is there; with one, forward rows -> finalize (which
    leaves sum omega on the device) -> backward."""
    h = _BinaryLoss(logits, layout)
    t = _binary_target(target, h.n, h.c, h.h, h.w, h.dev)
    opt = _binary_options(pos_weight, pixel_weight, ignore_value, h.n, h.h, h.w, h.c, h.dev)
    return binary_step(h, t, opt, w_bce, w_dice, dice_eps)


def binary_step(h, t, opt, w_bce, w_dice, dice_eps):
    """binary_loss_and_dlogits on a _BinaryLoss plan with a target and options that are already checked (_binary_target,
    _binary_options): the networks check them before their forward pass and come here after it"""
    if w_dice == 0.0:
        wsum = h.binary_weight_sum(t, opt) if h.needs_wsum(opt) else None
        part = h.partials()
        dl = h.binary_backward(t, opt, wsum, None, w_bce, part=part)
        return h.finalize_weighted(part, w_bce, w_dice, dice_eps)[0], dl
    out, coef, wsum = h.finalize_weighted(h.binary_forward(t, opt, True), w_bce, w_dice, dice_eps)
    return out, h.binary_backward(t, opt, wsum if h.needs_wsum(opt) else None, coef, w_bce)


def binary_loss_only(h, target, w_bce, w_dice, dice_eps, opt):
    """[loss, bce, dice] of a _BinaryLoss plan without a backward pass; target: checked by _binary_target; opt:
    _binary_options(...) or None"""
    return h.finalize_weighted(h.binary_forward(target, opt, w_dice != 0.0), w_bce, w_dice, dice_eps)[0]


class _BinaryCrossEntropyDice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, layout, w_bce, w_dice, dice_eps, pos_weight, pixel_weight, ignore_value):
        h = _BinaryLoss(logits.detach(), layout)
        t = _binary_target(target, h.n, h.c, h.h, h.w, h.dev)
        ctx.opt = _binary_options(pos_weight, pixel_weight, ignore_value, h.n, h.h, h.w, h.c, h.dev)
        out, coef, wsum = h.finalize_weighted(h.binary_forward(t, ctx.opt, w_dice != 0.0), w_bce, w_dice, dice_eps)
        ctx.h, ctx.t, ctx.w_bce = h, t, w_bce
        ctx.wsum = wsum if h.needs_wsum(ctx.opt) else None
        ctx.coef = coef if w_dice != 0.0 else None
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        # the upstream gradient stays on the device: the kernel reads it, nothing synchronises
        g = dout.detach().to(torch.float32).contiguous()
        dl = ctx.h.binary_backward(ctx.t, ctx.opt, ctx.wsum, ctx.coef, ctx.w_bce, dloss=g)
        ctx.h = ctx.t = ctx.coef = ctx.opt = ctx.wsum = None
        return dl, None, None, None, None, None, None, None, None


def binary_cross_entropy_dice(logits, target, w_bce=1.0, w_dice=0.0, dice_eps=1e-7, pos_weight=None, pixel_weight=None,
                              ignore_value=None):
    """w_bce * BCE + w_dice * soft Dice of NCHW fp32 CUDA logits (B, C, H, W) -- C independent sigmoid channels -- against a
    uint8 or bool mask of the same shape ((B, H, W) is accepted for C == 1): a 0-d loss that autograd differentiates through
    the HIP backward kernel.  w_dice == 0 and no options: F.binary_cross_entropy_with_logits(logits, target.float()).
    A mask value that is neither 0 nor 1 (nor ignore_value) gives a NaN loss; at most 16 channels.

    pos_weight: fp32 device tensor of C entries (or a sequence of floats, converted on every call), torch's
    BCEWithLogitsLoss(pos_weight=); pixel_weight: fp32 device tensor (B, H, W), one value for all channels of a pixel, a
    constant of the loss; ignore_value: an int in [2, 255] or None -- a mask element that equals it counts nowhere and gets a
    gradient of exactly 0.  BCE = sum omega l / sum omega with omega = valid * pixel_weight; the Dice sums run over the valid
    elements, unweighted.  Everything ignored: NaN."""
    return _BinaryCrossEntropyDice.apply(logits, target, L.SEG_NCHW, float(w_bce), float(w_dice), float(dice_eps), pos_weight,
                                         pixel_weight, ignore_value)


class SegLossMixin:
    """forward_backward / loss / predict (the contracts of unet._EngineNet) for networks that return logits.  The class
    defines `_logits_nhwc(x)` -- its forward without the final NCHW conversion -- and `_head`, the attribute path of its
    class-head convolution."""
    _head = None

    def _classes(self) -> int:
        return self.get_submodule(self._head).out_channels

    def _run_logits(self, x):
        lg = self._logits_nhwc(x)
        ops.flush_counters()      # what ToNCHW.forward does at the end of forward(): num_batches_tracked += 1
        return lg

    def _options_for(self, x, class_weight, pixel_weight, ignore_index):
        """the weighted loss's options checked against the input's geometry, before the forward pass runs"""
        if x.dim() != 4:
            raise RuntimeError(f"expected a 4-D input, got {tuple(x.shape)}")
        return _options(class_weight, pixel_weight, ignore_index, x.shape[0], x.shape[2], x.shape[3], self._classes(), x.device)

    def forward_backward(self, x, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7, stage_hook=None, class_weight=None,
                         pixel_weight=None, ignore_index=None):
        """Training step without the optimizer: forward to the NHWC logits, the loss kernels, backward.  OVERWRITES the
        `.grad` of every parameter that requires one (existing tensors stay the same objects -- FusedSGD's flat views --
        missing ones are allocated; a parameter the loss does not reach gets zeros) and returns the device tensor
        [loss, ce, dice]; with w_dice == 0 the Dice entry is 0.  stage_hook is accepted for the engine networks' signature
        and ignored: there is one gradient bucket, which GradAllReducer.finish() sends after backward.
        class_weight / pixel_weight / ignore_index: the weighted loss of cross_entropy_dice, on the same NHWC logits."""
        if not self.training:
            raise RuntimeError("forward_backward needs train() mode (batch statistics)")
        _check_classes(self._classes())
        opt = self._options_for(x, class_weight, pixel_weight, ignore_index)
        if opt is not None:
            class_weight, pixel_weight = opt[0], opt[1]
        params = [p for p in self.parameters() if p.requires_grad]
        with torch.enable_grad():
            lg = self._run_logits(x)
        out, dl = loss_and_dlogits(lg, target, w_ce, w_dice, dice_eps, class_weight, pixel_weight, ignore_index)
        # autograd.grad + one multi-tensor copy: zeroing .grad and letting backward accumulate into it costs one add launch
        # per parameter (~150 on AttU_Net)
        grads = torch.autograd.grad(lg, params, dl, allow_unused=True)
        for p in params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
        used = [(p.grad, g) for p, g in zip(params, grads) if g is not None]
        if used:
            torch._foreach_copy_([d for d, _ in used], [g for _, g in used])
        unused = [p.grad for p, g in zip(params, grads) if g is None]
        if unused:
            torch._foreach_zero_(unused)
        return out

    @torch.no_grad()
    def loss(self, x, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7, class_weight=None, pixel_weight=None, ignore_index=None):
        """[loss, ce, dice] of the current mode's forward pass (no gradients; buffers move as in model(x))."""
        _check_classes(self._classes())
        opt = self._options_for(x, class_weight, pixel_weight, ignore_index)
        h = _Loss(self._run_logits(x), L.SEG_NHWC)
        return loss_only(h, target, w_ce, w_dice, dice_eps, opt)

    @torch.no_grad()
    def predict(self, x):
        """Class map (int64, B x H x W) of the current mode's forward: the first maximum of the logits wins, like
        model(x).argmax(1)."""
        _check_classes(self._classes())
        return _Loss(self._run_logits(x), L.SEG_NHWC).forward(want_argmax=True)[1]

    # ---- binary / multi-label head ----------------------------------------------------------------------------------------
    def _binary_options_for(self, x, pos_weight, pixel_weight, ignore_value):
        if x.dim() != 4:
            raise RuntimeError(f"expected a 4-D input, got {tuple(x.shape)}")
        return _binary_options(pos_weight, pixel_weight, ignore_value, x.shape[0], x.shape[2], x.shape[3], self._classes(),
                               x.device)

    def forward_backward_binary(self, x, target, w_bce=1.0, w_dice=0.0, dice_eps=1e-7, stage_hook=None, pos_weight=None,
                                pixel_weight=None, ignore_value=None):
        """forward_backward with the sigmoid head of binary_cross_entropy_dice on the NHWC logits: every output channel is
        its own mask, target is uint8 / bool (B, C, H, W) (or (B, H, W) for one channel).  Same contract: train mode, `.grad`
        overwritten in place, returns the device tensor [loss, bce, dice]; stage_hook is accepted and ignored."""
        if not self.training:
            raise RuntimeError("forward_backward_binary needs train() mode (batch statistics)")
        _check_classes(self._classes())
        opt = self._binary_options_for(x, pos_weight, pixel_weight, ignore_value)
        target = _binary_target(target, x.shape[0], self._classes(), x.shape[2], x.shape[3], x.device)
        params = [p for p in self.parameters() if p.requires_grad]
        with torch.enable_grad():
            lg = self._run_logits(x)
        out, dl = binary_step(_BinaryLoss(lg, L.SEG_NHWC), target, opt, w_bce, w_dice, dice_eps)
        grads = torch.autograd.grad(lg, params, dl, allow_unused=True)
        for p in params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
        used = [(p.grad, g) for p, g in zip(params, grads) if g is not None]
        if used:
            torch._foreach_copy_([d for d, _ in used], [g for _, g in used])
        unused = [p.grad for p, g in zip(params, grads) if g is None]
        if unused:
            torch._foreach_zero_(unused)
        return out

    @torch.no_grad()
    def loss_binary(self, x, target, w_bce=1.0, w_dice=0.0, dice_eps=1e-7, pos_weight=None, pixel_weight=None,
                    ignore_value=None):
        """[loss, bce, dice] of the current mode's forward pass (no gradients; buffers move as in model(x))."""
        _check_classes(self._classes())
        opt = self._binary_options_for(x, pos_weight, pixel_weight, ignore_value)
        target = _binary_target(target, x.shape[0], self._classes(), x.shape[2], x.shape[3], x.device)
        h = _BinaryLoss(self._run_logits(x), L.SEG_NHWC)
        return binary_loss_only(h, target, w_bce, w_dice, dice_eps, opt)

    @torch.no_grad()
    def predict_mask(self, x, threshold=0.5):
        """uint8 masks (B, C, H, W) of the current mode's forward: sigmoid(logit) >= threshold, evaluated as
        logit >= float32(log(threshold / (1 - threshold))) -- model(x) >= that value, exactly."""
        tau = mask_threshold(threshold)
        _check_classes(self._classes())
        return _BinaryLoss(self._run_logits(x), L.SEG_NHWC).binary_mask(tau)
