"""Cross-entropy + soft-Dice loss on network logits (csrc/seg_loss.hip), and the training extras of the logits networks.

The loss is the fused UNet head's (oracle/ref_cpu.py::loss_head_fwd / loss_head_bwd): CE = mean over pixels of
-log softmax[target], Dice = 1 - mean_c (2 I_c + eps) / (P_c + Y_c + eps), loss = w_ce CE + w_dice Dice.  The per-workgroup
rows of the loss kernels are reduced by oct_head_loss_finalize, so both heads share one definition.

  cross_entropy_dice(logits, target, ...)  NCHW fp32 logits (any network's output) -> 0-d differentiable loss; with
                                           w_dice == 0 a drop-in for F.cross_entropy(logits, target)
  SegLossMixin                             forward_backward / loss / predict for the networks that return logits
                                           (U_Net, AttU_Net, AttU_Net4, MGUNet, MGUNet_2, ReLayNet), on the NHWC logits the
                                           network writes: no NCHW copy, no ATen softmax / NLL
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


def loss_and_dlogits(logits_nhwc, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7):
    """Training head on NHWC logits: ([loss, ce, dice], dlogits).  Without a Dice term the backward pass also writes the CE
    rows (the logits are read once; the Dice entry is then 0); with one, forward rows -> finalize -> backward."""
    h = _Loss(logits_nhwc, L.SEG_NHWC)
    t = _target(target, h.n, h.h, h.w, h.dev)
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
    def forward(ctx, logits, target, layout, w_ce, w_dice, dice_eps):
        h = _Loss(logits.detach(), layout)
        t = _target(target, h.n, h.h, h.w, h.dev)
        part, _ = h.forward(t)
        out, coef = h.finalize(part, w_ce, w_dice, dice_eps)
        ctx.h, ctx.t, ctx.w_ce = h, t, w_ce
        ctx.coef = coef if w_dice != 0.0 else None
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        # the upstream gradient stays on the device: the kernel reads it, nothing synchronises
        g = dout.detach().to(torch.float32).contiguous()
        dl = ctx.h.backward(ctx.t, ctx.coef, ctx.w_ce, dloss=g)
        ctx.h = ctx.t = ctx.coef = None
        return dl, None, None, None, None, None


def cross_entropy_dice(logits, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7):
    """w_ce * CE + w_dice * soft Dice of NCHW fp32 CUDA logits (B, C, H, W) against int64 labels (B, H, W): a 0-d loss
    that autograd differentiates through the HIP backward kernel.  w_dice == 0: F.cross_entropy(logits, target).
    A label outside [0, C) gives a NaN loss (torch raises there); at most 16 classes."""
    return _CrossEntropyDice.apply(logits, target, L.SEG_NCHW, float(w_ce), float(w_dice), float(dice_eps))


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

    def forward_backward(self, x, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7, stage_hook=None):
        """Training step without the optimizer: forward to the NHWC logits, the loss kernels, backward.  OVERWRITES the
        `.grad` of every parameter that requires one (existing tensors stay the same objects -- FusedSGD's flat views --
        missing ones are allocated; a parameter the loss does not reach gets zeros) and returns the device tensor
        [loss, ce, dice]; with w_dice == 0 the Dice entry is 0.  stage_hook is accepted for the engine networks' signature
        and ignored: there is one gradient bucket, which GradAllReducer.finish() sends after backward."""
        if not self.training:
            raise RuntimeError("forward_backward needs train() mode (batch statistics)")
        _check_classes(self._classes())
        params = [p for p in self.parameters() if p.requires_grad]
        with torch.enable_grad():
            lg = self._run_logits(x)
        out, dl = loss_and_dlogits(lg, target, w_ce, w_dice, dice_eps)
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
    def loss(self, x, target, w_ce=1.0, w_dice=0.0, dice_eps=1e-7):
        """[loss, ce, dice] of the current mode's forward pass (no gradients; buffers move as in model(x))."""
        _check_classes(self._classes())
        h = _Loss(self._run_logits(x), L.SEG_NHWC)
        part, _ = h.forward(_target(target, h.n, h.h, h.w, h.dev))
        return h.finalize(part, w_ce, w_dice, dice_eps)[0]

    @torch.no_grad()
    def predict(self, x):
        """Class map (int64, B x H x W) of the current mode's forward: the first maximum of the logits wins, like
        model(x).argmax(1)."""
        _check_classes(self._classes())
        return _Loss(self._run_logits(x), L.SEG_NHWC).forward(want_argmax=True)[1]
