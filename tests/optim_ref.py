"""float64 restatements of the optimizer layer (TEST INFRASTRUCTURE ONLY): Adam / AdamW as csrc/optim.hip evaluates them, the
clip coefficient of oct_grad_norm, the per-chunk weight-decay mask, and the rounding bounds the GPU tests hold the kernels to.
tests/test_optim_cpu.py pins the restatements to torch.optim.Adam / AdamW and torch.nn.utils.clip_grad_norm_ in float64.

Rounding bounds (adam_bounds).  Every fp32 rounding is counted as ONE ulp of the largest intermediate of its output -- twice its
worst case, the convention of test_gpu_bn.sgd_bounds.  The counts are read off adam_elem in csrc/optim.hip:

  g'  3 roundings: the scalar grad_scale * *dev_scale, g * that, fma(wd, p, .) (coupled decay).       G = |g gs| + |wd p|
  m   those 3, (1-b1) * g', fma(b1, m, .): 5 ulp of max(G, |m|, |m'|); b1, 1-b1 < 1 amplify nothing.
  v   the error of g' (3 ulp(G)) passes through the square: 2 G * 3 ulp(G) <= 6 * 2^-23 G^2 < 12 ulp(G^2) (ulp(x) > 2^-24 x);
      then g' * g', (1-b2) * ., fma(b2, v, .): 15 ulp of max(G^2, |v|, |v'|).
  p   decoupled decay p * (1 - lr wd): 1 ulp(p).  Denominator d = fma(sqrt(v'), inv_sqrt_bc2, eps): the error of v' through the
      square root, |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b) (sqrt|a - b| where b = 0), + 1 ulp(sqrt v'), times inv_sqrt_bc2,
      + 1 ulp(d).  Where g' cancels (|g'| << G: the decay term against the gradient) 15 ulp(G^2) says nothing about a v' of the
      size of g'^2, so the denominator takes the error of v' as it arises instead: e_g = 3 ulp(G) enters the square as
      2 |g'| e_g + e_g^2, times (1-b2), + the same 3 roundings as ulps of max((|g'| + e_g)^2, |v|, |v'|) -- the smaller of the
      two bounds, both of which hold.  Quotient
      q = m' / d: (e_m + |q| e_d) / (d - e_d) + 1 ulp(q).  Update fma(-step_size, q, p): step_size * e_q + 1 ulp of
      max(|p|, |step_size q|, |p'|).
Nothing here is fitted to what a kernel returns.
"""
import numpy as np
import torch

from oracle.bounds import ulp

CHUNK = 64          # floats per decay-mask byte (optim._ALIGN)


def f32(v):
    return float(np.float32(v))


def _f64(a):
    return np.asarray(a, np.float64)


def bias_corrections(lr, b1, b2, t):
    """step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1 / sqrt(1 - b2^t), float64"""
    return lr / (1.0 - b1 ** t), 1.0 / (1.0 - b2 ** t) ** 0.5


def scalars(lr, b1, b2, eps, wd, t, fp32=True):
    """The derived scalars of one step.  fp32=True: as the kernel receives them -- lr, betas, eps, wd are fp32 values, the derived
    ones 1 - beta and 1 - lr wd are computed in float64 from those and rounded once (the library's host code), the bias
    corrections come from the unrounded hyper-parameters (the caller's host code).  fp32=False: everything stays float64 (the torch comparison)."""
    r = f32 if fp32 else float
    ss, isb2 = bias_corrections(lr, b1, b2, t)      # from the hyper-parameters as given, as torch and optim.FusedAdam do
    lr, b1, b2, eps, wd = r(lr), r(b1), r(b2), r(eps), r(wd)
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, omb1=r(1.0 - b1), omb2=r(1.0 - b2), decay=r(1.0 - lr * wd),
                step_size=r(ss), isb2=r(isb2))


def expand_mask(mask, n):
    """per-element 0/1 from one byte per CHUNK floats (None: all ones)"""
    if mask is None:
        return np.ones(n, bool)
    return np.repeat(np.asarray(mask) != 0, CHUNK)[:n]


def chunk_mask(offsets, numels, total, excluded):
    """one byte per CHUNK floats: 0 over the whole (padded) span of every parameter i with excluded[i], 1 elsewhere"""
    assert total % CHUNK == 0 and all(o % CHUNK == 0 for o in offsets)
    mask = np.ones(total // CHUNK, np.uint8)
    ends = list(offsets[1:]) + [total]
    for o, e, x in zip(offsets, ends, excluded):
        if x:
            mask[o // CHUNK:e // CHUNK] = 0
    return mask


def adam_step(p, g, m, v, sc, decoupled, gscale=1.0, coef=None, mask=None):
    """One Adam (decoupled=False) / AdamW (True) step in float64.  Returns (p', m', v', parts); parts holds the intermediates the
    bounds need."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    wd = np.where(expand_mask(mask, p.size).reshape(p.shape), sc["wd"], 0.0)
    gs = float(gscale) * (1.0 if coef is None else float(coef))
    gr = g * gs
    G = np.abs(gr)
    pv = p
    if decoupled:
        pv = np.where(wd != 0, p * sc["decay"], p)
    else:
        gr = gr + wd * p
        G = G + np.abs(wd * p)
    mn = sc["b1"] * m + sc["omb1"] * gr
    vn = sc["b2"] * v + sc["omb2"] * gr * gr
    root = np.sqrt(vn)
    den = root * sc["isb2"] + sc["eps"]
    q = mn / den
    pn = pv - sc["step_size"] * q
    return pn, mn, vn, dict(G=G, gr=gr, pv=pv, root=root, den=den, q=q, decayed=decoupled & (wd != 0))


def adam_bounds(p, g, m, v, sc, decoupled, gscale=1.0, coef=None, mask=None):
    """(p', m', v', tol_p, tol_m, tol_v) -- see the module docstring for the derivation"""
    pn, mn, vn, x = adam_step(p, g, m, v, sc, decoupled, gscale, coef, mask)
    p, m, v = _f64(p), _f64(m), _f64(v)
    big = np.maximum.reduce
    tol_m = 5 * ulp(big([x["G"], np.abs(m), np.abs(mn)]), "f32")
    tol_v = 15 * ulp(big([x["G"] ** 2, np.abs(v), np.abs(vn)]), "f32")
    e_g = 3 * ulp(x["G"], "f32")
    a_g = np.abs(x["gr"])
    e_v = np.minimum(tol_v, sc["omb2"] * (2 * a_g * e_g + e_g ** 2) + 3 * ulp(big([(a_g + e_g) ** 2, np.abs(v), np.abs(vn)]), "f32"))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_root = np.where(vn > 0, e_v / np.where(vn > 0, x["root"], 1.0), np.sqrt(e_v)) + ulp(x["root"], "f32")
    e_den = sc["isb2"] * e_root + ulp(x["den"], "f32")
    den_lo = x["den"] - e_den
    assert (den_lo > 0).all(), "the denominator is not resolved: v' is too close to 0 for this bound"
    e_q = (tol_m + np.abs(x["q"]) * e_den) / den_lo + ulp(x["q"], "f32")
    e_pv = np.where(x["decayed"], ulp(p, "f32"), 0.0)
    tol_p = e_pv + sc["step_size"] * e_q + ulp(big([np.abs(x["pv"]), np.abs(sc["step_size"] * x["q"]), np.abs(pn)]), "f32")
    return pn, mn, vn, tol_p, tol_m, tol_v


def clip(g, gscale, max_norm):
    """(norm, coef) of torch.nn.utils.clip_grad_norm_ on g * gscale, float64: coef = min(1, max_norm / (norm + 1e-6)); a NaN norm
    gives a NaN coefficient, an infinite one 0 (torch.clamp)."""
    x = _f64(g) * float(gscale)
    with np.errstate(invalid="ignore", over="ignore"):
        norm = float(np.sqrt(np.sum(x * x)))
        c = float(max_norm) / (norm + 1e-6)
    return norm, (1.0 if c > 1.0 else c)


# ---- the free-running recurrence of the 50-step test: gradients that do not depend on the parameters ----
REC_STEPS, REC_LR, REC_WD = 50, 1e-3, 1e-2


def recurrence_inputs(n, steps=REC_STEPS):
    rng = np.random.default_rng(20250117)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 1e-2).astype(np.float32) for _ in range(steps)]
    return p0, grads


def torch_adamw_recurrence(p0, grads, dtype):
    """torch.optim.AdamW (CPU, foreach=False) in `dtype` over the fp32 inputs; the final parameters as float64"""
    p = torch.from_numpy(p0.copy()).to(dtype).requires_grad_(True)         # (a same-dtype .to() would alias p0)
    opt = torch.optim.AdamW([p], lr=REC_LR, weight_decay=REC_WD, foreach=False)
    for g in grads:
        p.grad = torch.from_numpy(g.copy()).to(dtype)
        opt.step()
    return p.detach().double().numpy()
