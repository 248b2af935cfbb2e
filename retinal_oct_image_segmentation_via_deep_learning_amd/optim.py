"""Fused optimizers over ONE flat fp32 parameter buffer: SGD (torch.optim.SGD semantics: momentum, dampening 0, no
nesterov) and Adam / AdamW (torch.optim.Adam / AdamW, single tensor, no amsgrad), both with optional global-norm gradient
clipping (torch.nn.utils.clip_grad_norm_) and torch-layout state dicts.  Parameters and their .grad become views into two
flat buffers, so the optimizer step is a single HIP kernel and the data-parallel exchange a few contiguous slices.

`FlatParams` is the layout alone (host logic, any device -- the gloo tests build it on CPU): offsets, the per-chunk
weight-decay mask, and splitting / joining flat state buffers for checkpoints.  The `step` methods are HIP kernels
(csrc/bn.hip, csrc/optim.hip) and refuse CPU tensors: there is no CPU fallback.

Not provided (the keywords raise): amsgrad, nesterov, maximize, per-group learning rates, capturable / graph-captured
steps -- the step stays outside the HIP graph of ddp.DataParallelTrainer."""
from __future__ import annotations

import torch

from . import _lib as L

_ALIGN = 64  # floats; one decay-mask byte of csrc/optim.hip covers one such chunk

NO_DECAY_1D = lambda name, p: p.ndim <= 1  # noqa: E731  -- BatchNorm weights / biases and convolution biases


class FlatParams:
    """Re-homes parameters (and their gradients) as views into two flat fp32 buffers, in the order
    given -- `model.named_parameters()` order, i.e. the reference's construction order."""

    def __init__(self, named_params):
        named = [(n, p) for n, p in named_params]
        if not named:
            raise ValueError("no parameters")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        dev = self.params[0].device
        self.offsets, total = [], 0
        for p in self.params:
            if p.dtype != torch.float32:
                raise L.OctError("flat parameter buffer needs fp32 parameters")
            self.offsets.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.total = total
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.flat_p[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat_p[o:o + n].view(p.shape)
            p.grad = self.flat_g[o:o + n].view(p.shape)

    def span(self, name: str):
        """[lo, hi) of one parameter inside the flat buffers (hi includes the alignment padding)."""
        i = self.names.index(name)
        hi = self.offsets[i + 1] if i + 1 < len(self.offsets) else self.total
        return self.offsets[i], hi


    def decay_mask(self, no_decay=None) -> torch.Tensor:
        """uint8 [total / 64] on the CPU: 0 for every 64-float chunk of a parameter that `no_decay(name, param)` selects,
        1 elsewhere.  Spans start on chunk boundaries, so no chunk belongs to two parameters."""
        mask = torch.ones(self.total // _ALIGN, dtype=torch.uint8)
        if no_decay is not None:
            for name, p in zip(self.names, self.params):
                if no_decay(name, p):
                    lo, hi = self.span(name)
                    mask[lo // _ALIGN:hi // _ALIGN] = 0
        return mask

    def split(self, flat: torch.Tensor):
        """Per-parameter copies (parameter order, parameter shapes) of a flat buffer laid out like flat_p."""
        if flat.numel() != self.total:
            raise ValueError(f"flat buffer of {flat.numel()} elements, layout has {self.total}")
        return [flat[o:o + p.numel()].detach().clone().view(p.shape) for p, o in zip(self.params, self.offsets)]

    def join(self, tensors, out: torch.Tensor | None = None) -> torch.Tensor:
        """The reverse of split(): one flat fp32 buffer (a new one on flat_p's device, or `out`) with the alignment padding
        written as zero.  ValueError on a count or shape mismatch."""
        tensors = list(tensors)
        if len(tensors) != len(self.params):
            raise ValueError(f"{len(tensors)} tensors for {len(self.params)} parameters")
        for name, p, t in zip(self.names, self.params, tensors):
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"{name}: shape {tuple(t.shape)} does not match the parameter's {tuple(p.shape)}")
        if out is None:
            out = torch.empty(self.total, dtype=torch.float32, device=self.flat_p.device)
        elif out.numel() != self.total:
            raise ValueError(f"flat buffer of {out.numel()} elements, layout has {self.total}")
        out.zero_()
        for p, o, t in zip(self.params, self.offsets, tensors):
            out[o:o + p.numel()].copy_(t.detach().reshape(-1))
        return out


def _refuse(kind, kw):
    for k, v in kw.items():
        if k in ("amsgrad", "nesterov", "maximize", "capturable", "differentiable") and not v:
            continue
        if k in ("foreach", "fused") and v is None:
            continue
        raise NotImplementedError(f"{kind}: {k}={v!r} is not provided (no amsgrad, nesterov, maximize, capturable steps or "
                                  "per-group options)")


class _FlatOptimizer:
    """What FusedSGD and FusedAdam share: re-homing, zero_grad, the clip call and the torch-layout state dict."""

    def _init_layout(self, params, max_grad_norm, no_decay):
        params = list(params)
        if params and isinstance(params[0], dict):
            raise NotImplementedError(f"{type(self).__name__}: parameter groups (per-group learning rates) are not provided")
        if params and isinstance(params[0], tuple):
            named = params
        else:
            named = [(f"p{i}", p) for i, p in enumerate(params)]
        if not named:
            raise ValueError("no parameters")
        if named[0][1].device.type != "cuda":
            raise L.OctError(f"{type(self).__name__} needs device parameters (no CPU fallback)")
        self.layout = FlatParams(named)
        self.params = self.layout.params
        self.flat_p, self.flat_g = self.layout.flat_p, self.layout.flat_g
        self.steps = 0
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        dev = self.flat_p.device
        # {norm, clip coefficient} of the last clipped step, written by oct_grad_norm: reading it is the caller's sync
        self.last_grad_norm = torch.zeros(2, dtype=torch.float32, device=dev) if max_grad_norm is not None else None
        self._norm_rows = None
        if max_grad_norm is not None:
            self._norm_rows = torch.zeros(L.lib().oct_grad_norm_blocks(self.flat_g.numel()), dtype=torch.float64, device=dev)
        self.no_decay = no_decay
        self.decay_mask = self.layout.decay_mask(no_decay).to(dev) if no_decay is not None else None

    def zero_grad(self, set_to_none: bool = False):
        """Gradients are overwritten (not accumulated) by UNet.forward_backward; kept for API parity."""
        self.flat_g.zero_()

    def _clip(self, grad_scale: float, stream):
        """Launches the norm of flat_g * grad_scale; returns the device pointer of the clip coefficient (None: no clipping)."""
        if self.max_grad_norm is None:
            return None
        L.check(L.lib().oct_grad_norm(self.flat_g.data_ptr(), self.flat_g.numel(), grad_scale, self.max_grad_norm,
                                      self._norm_rows.data_ptr(), self.last_grad_norm.data_ptr(), stream), "oct_grad_norm")
        return self.last_grad_norm.data_ptr() + 4

    def _dict(self, group: dict, state_buffers: dict, extra: dict) -> dict:
        n = len(self.params)
        parts = {k: self.layout.split(b) for k, b in state_buffers.items()}
        state = {}
        if parts or extra:
            for i in range(n):
                state[i] = {k: v.clone() if torch.is_tensor(v) else v for k, v in extra.items()}
                state[i].update({k: parts[k][i] for k in parts})
        group = dict(group)
        group["max_grad_norm"] = self.max_grad_norm
        group["params"] = list(range(n))
        return {"state": state, "param_groups": [group]}

    def _check_dict(self, sd: dict, keys):
        """One group over all parameters, state for none or for all of them with the parameters' shapes."""
        groups = sd["param_groups"]
        n = len(self.params)
        if len(groups) != 1 or len(groups[0]["params"]) != n:
            raise ValueError(f"state dict with {[len(g['params']) for g in groups]} parameters per group; this optimizer has "
                             f"one group of {n}")
        state = sd["state"]
        if state and sorted(state.keys()) != list(range(n)):
            raise ValueError(f"state for {len(state)} of {n} parameters")
        for k in keys:
            for i, p in enumerate(self.params):
                if state and torch.is_tensor(state[i].get(k)) and tuple(state[i][k].shape) != tuple(p.shape):
                    raise ValueError(f"{self.layout.names[i]}: {k} of shape {tuple(state[i][k].shape)} does not match the "
                                     f"parameter's {tuple(p.shape)}")
        return groups[0], state


class FusedSGD(_FlatOptimizer):
    def __init__(self, params, lr: float, momentum: float = 0.0, weight_decay: float = 0.0, max_grad_norm=None, no_decay=None,
                 **unsupported):
        _refuse("FusedSGD", unsupported)
        self._init_layout(params, max_grad_norm, no_decay)
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.buf = torch.zeros_like(self.flat_p) if momentum != 0.0 else None

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        stream = torch.cuda.current_stream().cuda_stream
        first = 1 if self.steps == 0 else 0
        if self.max_grad_norm is None and self.decay_mask is None:
            L.check(L.lib().oct_sgd_step(self.flat_p.data_ptr(), self.flat_g.data_ptr(), L.ptr(self.buf),
                                         self.flat_p.numel(), self.lr, self.momentum, self.weight_decay, grad_scale,
                                         first, stream),
                    "oct_sgd_step")
        else:
            coef = self._clip(grad_scale, stream)
            L.check(L.lib().oct_sgd_step_scaled(self.flat_p.data_ptr(), self.flat_g.data_ptr(), L.ptr(self.buf),
                                                self.flat_p.numel(), self.lr, self.momentum, self.weight_decay, grad_scale,
                                                first, coef, L.ptr(self.decay_mask), stream),
                    "oct_sgd_step_scaled")
        self.steps += 1
        L.param_generation[0] += 1  # packed-weight caches must notice the raw-pointer update

    def state_dict(self) -> dict:
        """torch.optim.SGD's layout; "momentum_buffer" is absent before the first step (and without momentum).  The group
        carries two keys torch does not know and ignores: "max_grad_norm" and "steps"."""
        group = {"lr": self.lr, "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay, "nesterov": False,
                 "maximize": False, "foreach": None, "differentiable": False, "fused": None, "steps": self.steps}
        bufs = {"momentum_buffer": self.buf} if self.buf is not None and self.steps > 0 else {}
        return self._dict(group, bufs, {})

    def load_state_dict(self, sd: dict):
        group, state = self._check_dict(sd, ("momentum_buffer",))
        _refuse("FusedSGD", {k: group[k] for k in ("nesterov", "maximize") if k in group})
        if group.get("dampening", 0) != 0:
            raise NotImplementedError("FusedSGD: dampening is not provided")
        momentum = group["momentum"]
        have = bool(state) and all(torch.is_tensor(state[i].get("momentum_buffer")) for i in range(len(self.params)))
        if momentum != 0.0:
            if self.buf is None:
                self.buf = torch.zeros_like(self.flat_p)
            if have:
                self.layout.join([state[i]["momentum_buffer"] for i in range(len(self.params))], out=self.buf)
            else:
                self.buf.zero_()
        else:
            self.buf = None
        self.lr, self.momentum, self.weight_decay = group["lr"], momentum, group["weight_decay"]
        # the first-step flag: a momentum buffer exists exactly when a step has been taken
        self.steps = int(group["steps"]) if "steps" in group else (1 if have else 0)
        if momentum != 0.0 and not have:
            self.steps = 0


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam (decoupled=False: L2 decay added to the gradient) or AdamW (decoupled=True) over the flat buffers,
    one kernel per step (oct_adam_step).  `lr` is a plain attribute: a schedule assigns `opt.lr` between steps.
    no_decay(name, param) -> bool excludes parameters from weight decay (NO_DECAY_1D: BatchNorm parameters and biases).
    max_grad_norm clips the global L2 norm of the (scaled) gradient as clip_grad_norm_ does, on the device: `step()` then
    issues three launches and no synchronisation; `last_grad_norm` holds {norm, coefficient} as a device tensor."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled: bool = False, max_grad_norm=None, no_decay=None, **unsupported):
        _refuse(type(self).__name__, unsupported)
        b1, b2 = betas
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas {betas!r} outside [0, 1)")
        if not eps > 0.0:
            raise ValueError("eps must be positive")
        if lr < 0.0 or weight_decay < 0.0:
            raise ValueError("lr and weight_decay must not be negative")
        self._init_layout(params, max_grad_norm, no_decay)
        self.lr, self.betas, self.eps, self.weight_decay, self.decoupled = lr, (float(b1), float(b2)), eps, weight_decay, decoupled
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)

    @staticmethod
    def bias_corrections(lr: float, betas, t: int):
        """(step_size, inv_sqrt_bc2) of step t >= 1 in float64, as torch's single-tensor Adam computes them."""
        b1, b2 = betas
        return lr / (1.0 - b1 ** t), 1.0 / (1.0 - b2 ** t) ** 0.5

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0):
        stream = torch.cuda.current_stream().cuda_stream
        coef = self._clip(grad_scale, stream)
        step_size, isb2 = self.bias_corrections(self.lr, self.betas, self.steps + 1)
        L.check(L.lib().oct_adam_step(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                                      self.exp_avg_sq.data_ptr(), self.flat_p.numel(), self.lr, self.betas[0], self.betas[1],
                                      self.eps, self.weight_decay, 1 if self.decoupled else 0, step_size, isb2, grad_scale,
                                      coef, L.ptr(self.decay_mask), stream),
                "oct_adam_step")
        self.steps += 1
        L.param_generation[0] += 1  # packed-weight caches must notice the raw-pointer update

    def state_dict(self) -> dict:
        """torch.optim.Adam's layout ("step" a float tensor); empty state before the first step.  The group carries one key
        torch does not know and ignores: "max_grad_norm"."""
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": self.decoupled}
        if self.steps == 0:
            return self._dict(group, {}, {})
        return self._dict(group, {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq},
                          {"step": torch.tensor(float(self.steps), dtype=torch.float32)})

    def load_state_dict(self, sd: dict):
        group, state = self._check_dict(sd, ("exp_avg", "exp_avg_sq"))
        _refuse(type(self).__name__, {k: group[k] for k in ("amsgrad", "maximize", "capturable") if k in group})
        n = len(self.params)
        if state:
            steps = {int(float(state[i]["step"])) for i in range(n)}
            if len(steps) != 1:
                raise ValueError(f"parameters at different steps {sorted(steps)}: one step count for the flat buffer")
            self.layout.join([state[i]["exp_avg"] for i in range(n)], out=self.exp_avg)
            self.layout.join([state[i]["exp_avg_sq"] for i in range(n)], out=self.exp_avg_sq)
            self.steps = steps.pop()
        else:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.steps = 0
        self.lr, self.eps, self.weight_decay = group["lr"], group["eps"], group["weight_decay"]
        self.betas = (float(group["betas"][0]), float(group["betas"][1]))
        self.decoupled = bool(group.get("decoupled_weight_decay", self.decoupled))


class FusedAdamW(FusedAdam):
    """FusedAdam with torch.optim.AdamW's defaults: decoupled decay of 1e-2."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm=None, no_decay=None, **unsupported):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True,
                         max_grad_norm=max_grad_norm, no_decay=no_decay, **unsupported)
