"""numpy float64 restatements of the BatchNorm / ReLU / 2x2 max-pool / optimizer kernels of csrc/bn.hip (and
oct_reduce_bias_partials of csrc/wgrad.hip), stage by stage, written from the contracts in include/oct_hip.h
(TEST INFRASTRUCTURE ONLY).  Pinned to torch's float64 CPU operators by tests/test_oracle_bn.py.

Inputs and outputs are the tensors the kernels read and write: NHWC activations, per-channel vectors, partial rows
[nblocks][2][c].  Everything is evaluated in float64 on the values given.  Two places are part of the contract and are
restated as the kernels do them:

* the pre-activation that decides a mask or a pool route is z = fma(y, scale, shift) rounded ONCE to fp32 (`z32`): a
  mask is the sign of z (which one rounding keeps) and a route is a comparison of z values, so both are selections;
* a gradient that the kernels hold in the storage type (g, and the PReLU slope branch da * alpha) is rounded to that type
  (`store`) BEFORE it enters the sums and the apply, so that dy is consistent with the g a consumer sees.
"""
import numpy as np

from . import ref_stream as RS


def _f64(a):
    return np.asarray(a, np.float64)


def _ident(v):
    return v


def z32(y, scale, shift):
    """fma(y, scale, shift) rounded once to fp32 (the product of two fp32 values is exact in float64)"""
    with np.errstate(invalid="ignore"):
        return (_f64(y) * _f64(scale) + _f64(shift)).astype(np.float32).astype(np.float64)


# ---- oct_bn_finalize: partial rows -> statistics, fused affine coefficients, running statistics ----
def bn_finalize(rows, count, gamma, beta, eps, momentum=0.1, conv_bias=None, running_mean=None, running_var=None):
    """rows [nblocks][2][c] (sum, sum of squares).  Biased variance normalises, unbiased goes into running_var; a conv
    bias in front of the BN only shifts the running mean.  Returns a dict; 'running_*' are None when not given."""
    rows = _f64(rows)
    s1, s2 = rows[:, 0].sum(0), rows[:, 1].sum(0)
    count = float(count)
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + float(eps))
    scale = _f64(gamma) * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=_f64(beta) - mean * scale, ex2=s2 / count,
               running_mean=None, running_var=None)
    if running_mean is not None:
        unbiased = var * (count / (count - 1.0)) if count > 1.0 else var
        mb = mean + (_f64(conv_bias) if conv_bias is not None else 0.0)
        m = float(momentum)
        out["running_mean"] = (1.0 - m) * _f64(running_mean) + m * mb
        out["running_var"] = (1.0 - m) * _f64(running_var) + m * unbiased
    return out


# ---- oct_bn_eval_coeffs: z = scale * (y + conv_bias - running_mean) + beta ----
def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps, conv_bias=None):
    scale = _f64(gamma) / np.sqrt(_f64(running_var) + float(eps))
    m = _f64(running_mean) - (_f64(conv_bias) if conv_bias is not None else 0.0)
    return scale, _f64(beta) - m * scale


# ---- oct_bn_relu_fwd / oct_bn_relu_pool_fwd ----
def bn_relu(y, scale, shift):
    """returns (a, terms, z): a = relu(y*scale + shift), NaN kept (torch.relu); terms = |y*scale| + |shift|"""
    ys = _f64(y) * _f64(scale)
    with np.errstate(invalid="ignore"):
        z = ys + _f64(shift)
        a = np.maximum(z, 0.0)             # np.maximum propagates NaN
    return a, np.abs(ys) + np.abs(_f64(shift)) + np.zeros_like(ys), z


def bn_relu_pool(y, scale, shift):
    """returns (pooled, terms, a): MaxPool2d(2, 2) over relu(y*scale + shift); a window that holds a NaN pools to NaN"""
    a, terms, _ = bn_relu(y, scale, shift)
    pooled, code = RS.maxpool(a, 2)
    return pooled, RS.window_gather(terms, code, 2), a


# ---- oct_dact_bn_reduce ----
def pool_route(dpool, y, scale, shift):
    """dpool scattered to the FIRST maximum (row-major) of each activated 2x2 window -- ATen's max_pool2d backward"""
    a = np.maximum(z32(y, scale, shift), 0.0)
    win = RS._windows(a, 2)
    best, code = win[..., 0, :], np.zeros(win[..., 0, :].shape, np.int64)
    for q in range(1, 4):
        take = win[..., q, :] > best       # strict: the first maximum wins
        best = np.where(take, win[..., q, :], best)
        code = np.where(take, q, code)
    n, h, w, _ = np.shape(y)
    return RS.window_scatter(_f64(dpool), code, 2, h, w)


def dact_bn_reduce(da, dpool, y, scale, shift, mean, invstd, store=_ident):
    """g = store((da + route(dpool)) * [z > 0]); s1 = sum g, s2 = sum g * xhat over the pixels, xhat = (y - mean) * invstd.
    da or dpool may be None.  Returns dict(g, s1, s2, t1, t2, count): t* = sum |terms| and count = terms per output."""
    y = _f64(y)
    d = np.zeros_like(y) if da is None else _f64(da).copy()
    if dpool is not None:
        d = d + pool_route(dpool, y, scale, shift)
    g = _f64(store(np.where(z32(y, scale, shift) > 0, d, 0.0)))
    return _sums(g, y, mean, invstd)


def _sums(g, y, mean, invstd):
    gx = g * ((y - _f64(mean)) * _f64(invstd))
    ax = (0, 1, 2)
    return dict(g=g, s1=g.sum(ax), s2=gx.sum(ax), t1=np.abs(g).sum(ax), t2=np.abs(gx).sum(ax),
                count=g.shape[0] * g.shape[1] * g.shape[2])


# ---- oct_bn_bwd_finalize ----
def bn_bwd_finalize(rows, count, gamma, mean, invstd, dgamma=None, dbeta=None, accumulate=False):
    """rows [nblocks][2][c] (sum g, sum g*xhat) -> dgamma, dbeta and coef[3][c] of dy = k0*g + k1*y + k2:
    dy = gamma*invstd * (g - sum(g)/N - xhat * sum(g*xhat)/N)"""
    rows = _f64(rows)
    s1, s2 = rows[:, 0].sum(0), rows[:, 1].sum(0)
    a = _f64(gamma) * _f64(invstd)
    mg, mgx = s1 / float(count), s2 / float(count)
    k1 = -a * _f64(invstd) * mgx
    k2 = -a * mg - k1 * _f64(mean)
    dg, db = s2, s1
    if accumulate:
        dg, db = _f64(dgamma) + s2, _f64(dbeta) + s1
    return dict(dgamma=dg, dbeta=db, coef=np.stack([a, k1, k2]), s1=s1, s2=s2, k2_terms=np.abs(a * mg) + np.abs(k1 * _f64(mean)))


# ---- oct_bn_bwd_apply / _to / _pool ----
def bn_bwd_apply(g, y, coef, scale=None, shift=None):
    """dy = k0*g + k1*y + k2; with scale / shift, g holds dA and the ReLU mask [z > 0] is re-derived first.
    Returns (dy, terms)."""
    g, y, coef = _f64(g), _f64(y), _f64(coef)
    if scale is not None:
        g = np.where(z32(y, scale, shift) > 0, g, 0.0)
    return coef[0] * g + coef[1] * y + coef[2], np.abs(coef[0] * g) + np.abs(coef[1] * y) + np.abs(coef[2])


def bn_bwd_apply_pool(da, dpool, y, scale, shift, coef, store=_ident):
    """the routed and masked g of dact_bn_reduce (rounded to the storage type), never stored, then the apply"""
    g = dact_bn_reduce(da, dpool, y, scale, shift, 0.0, 1.0, store)["g"]
    return bn_bwd_apply(g, y, coef)


# ---- PReLU in place of the ReLU mask: oct_dact_bn_reduce_prelu / oct_bn_bwd_apply_prelu_to ----
def prelu_dz(da, y, scale, shift, alpha, store=_ident):
    """dz = dA where z > 0, else store(dA * alpha): the slope branch is taken at z == 0 (ATen); returns (dz, z)"""
    z = z32(y, scale, shift)
    da = _f64(da)
    return np.where(z > 0, da, _f64(store(da * float(alpha)))), z


def dact_bn_reduce_prelu(da, y, scale, shift, alpha, mean, invstd, store=_ident):
    """sums of dz and dz * xhat, and dalpha = sum dA * z * [z <= 0] (z as the kernel holds it: one fp32 rounding)"""
    dz, z = prelu_dz(da, y, scale, shift, alpha, store)
    out = _sums(dz, _f64(y), mean, invstd)
    t = np.where(z > 0, 0.0, _f64(da) * z)
    out.update(dalpha=t.sum(), dalpha_terms=np.abs(t).sum(), z=z)
    return out


def bn_bwd_apply_prelu(da, y, coef, scale, shift, alpha, store=_ident):
    dz, _ = prelu_dz(da, y, scale, shift, alpha, store)
    return bn_bwd_apply(dz, y, coef)


# ---- oct_reduce_bias_partials ----
def reduce_bias_partials(part, channels, dbias=None, accumulate=False):
    """part [nparts][rows], rows = fold * channels: dbias[c] (+)= sum over slabs and over the rows q = c (mod channels).
    Returns (dbias, terms, count)."""
    part = _f64(part)
    nparts, rows = part.shape
    p = part.reshape(nparts, rows // channels, channels)
    out, terms = p.sum((0, 1)), np.abs(p).sum((0, 1))
    if accumulate:
        out, terms = out + _f64(dbias), terms + np.abs(_f64(dbias))
    return out, terms, nparts * (rows // channels) + (1 if accumulate else 0)


# ---- oct_sgd_step: torch.optim.SGD (dampening 0, no nesterov) on a gradient pre-multiplied by grad_scale ----
def sgd_step(p, g, buf, lr, momentum, weight_decay, grad_scale, first):
    """returns (p_new, buf_new, mags): buf_new is buf itself (untouched, may be None) when momentum == 0.
    mags = sum of |addends| of the update direction, for error bounds."""
    p = _f64(p)
    gr = _f64(g) * float(grad_scale)
    mags = np.abs(gr)
    if weight_decay != 0:
        gr = float(weight_decay) * p + gr
        mags = mags + np.abs(float(weight_decay) * p)
    if momentum != 0:
        if not first:
            gr = float(momentum) * _f64(buf) + gr
            mags = mags + np.abs(float(momentum) * _f64(buf))
        buf = gr
    return p - float(lr) * gr, buf, mags
