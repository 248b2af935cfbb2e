"""numpy restatements of the streaming kernels of csrc/blocks.hip and oct_channel_sum (csrc/bn.hip), written from the
formulas in the kernels' header comments (TEST INFRASTRUCTURE ONLY).

Tensors are NHWC like the kernels'.  Arithmetic ops work in float64; selection / copy ops keep their input dtype (they
are exact in any precision).  Where the choice of sample is part of the contract (the bilinear source index), it is
computed in fp32 exactly as documented.  Pinned to torch's CPU operators by tests/test_oracle_stream.py.
"""
import numpy as np

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def _f64(a):
    return np.asarray(a, np.float64)


# ---- out = act(scale[c] * y + shift[c] (+ res)), the residual's deferred bias rounded to the storage type first ----
def affine_act(y, scale, shift, act, res=None, res_shift=None, store=None):
    """returns (out, terms): terms = sum of |addends| of the pre-activation, for error bounds.
    store: the storage-type rounding that (r + b) goes through when res_shift is given."""
    ys = _f64(y) * _f64(scale)
    z = ys + _f64(shift)
    terms = np.abs(ys) + np.abs(_f64(shift))
    if res is not None:
        r = _f64(res)
        if res_shift is not None:
            r = _f64(store(r + _f64(res_shift)))
        z = z + r
        terms = terms + np.abs(r)
    return activate(z, act), terms, z


def activate(z, act):
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-z))
    return z


def act_bwd(dout, out, act):
    """dz = dout * act'(z) through the stored output: relu -> [out > 0], sigmoid -> out (1 - out)"""
    d, o = _f64(dout), _f64(out)
    if act == ACT_RELU:
        return np.where(o > 0, d, 0.0)
    return d * o * (1.0 - o)


# ---- max-pooling: k x k windows, stride k, floor mode; torch's rule: a candidate wins when larger or NaN ----
def _windows(a, k):
    n, h, w, c = a.shape
    ho, wo = h // k, w // k
    win = a[:, :ho * k, :wo * k].reshape(n, ho, k, wo, k, c).transpose(0, 1, 3, 2, 4, 5)
    return win.reshape(n, ho, wo, k * k, c)


def maxpool(a, k):
    """returns (out, code): code = (iy - yo*k)*k + (ix - xo*k) of the winning tap"""
    a = np.asarray(a)
    win = _windows(a, k)
    m = np.full(win.shape[:3] + win.shape[4:], -np.inf, a.dtype)
    code = np.zeros(m.shape, np.int64)
    for q in range(k * k):
        v = win[..., q, :]
        take = (v > m) | np.isnan(v)
        m = np.where(take, v, m)
        code = np.where(take, q, code)
    return m, code


def maxpool_plane_index(code, k, w):
    """torch's MaxPool2d(return_indices=True) index iy*W + ix inside the (n, c) plane, from the window code"""
    _, ho, wo, _ = code.shape
    yo = np.arange(ho)[None, :, None, None]
    xo = np.arange(wo)[None, None, :, None]
    return (yo * k + code // k) * w + xo * k + code % k


def window_scatter(v, code, k, h=None, w=None):
    """MaxUnpool2d by window code (= max-pool backward): the value lands at its code, zeros elsewhere and outside every window"""
    v = np.asarray(v)
    n, ho, wo, c = v.shape
    h = ho * k if h is None else h
    w = wo * k if w is None else w
    out = np.zeros((n, h, w, c), v.dtype)
    for q in range(k * k):
        out[:, q // k:ho * k:k, q % k:wo * k:k] = np.where(code == q, v, 0)
    return out


def window_gather(x, code, k):
    """MaxUnpool2d backward by window code: v = x at the code of every window"""
    x = np.asarray(x)
    return np.take_along_axis(_windows(x, k), code[:, :, :, None, :], axis=3)[:, :, :, 0]


def index_scatter(v, idx, h, w):
    """out[n, idx, c] = v[n, p, c] for indices inside the plane [0, h*w); zeros elsewhere"""
    v = np.asarray(v)
    n, c = v.shape[0], v.shape[-1]
    out = np.zeros((n, h * w, c), v.dtype)
    vf, qf = v.reshape(n, -1, c), idx.reshape(n, -1, c)
    for img in range(n):
        for ch in range(c):
            q = qf[img, :, ch]
            ok = (q >= 0) & (q < h * w)
            out[img, q[ok], ch] = vf[img, ok, ch]
    return out.reshape(n, h, w, c)


def index_gather(x, idx):
    """v[n, p, c] = x[n, idx, c] (zero for an index outside the plane)"""
    x = np.asarray(x)
    n, h, w, c = x.shape
    qf = idx.reshape(n, -1, c)
    ok = (qf >= 0) & (qf < h * w)
    v = np.take_along_axis(x.reshape(n, h * w, c), np.where(ok, qf, 0), axis=1)
    return np.where(ok, v, 0).astype(x.dtype).reshape(idx.shape)


def depth_pool(p2):
    """p2: (nslab, 2, m) -> max over the pair: slice 1 wins when larger or NaN; returns (out, second)"""
    p2 = np.asarray(p2)
    a, b = p2[:, 0], p2[:, 1]
    second = (b > a) | np.isnan(b)
    return np.where(second, b, a), second


def depth_pool_bwd(p2, dout):
    _, second = depth_pool(p2)
    dout = np.asarray(dout)
    z = np.zeros_like(dout)
    return np.stack([np.where(second, z, dout), np.where(second, dout, z)], axis=1)


# ---- bilinear resize, align_corners=True ----
def bilinear_taps(n_in, n_out):
    """the documented fp32 source index: r = f32((in-1)/(out-1)) (0 for one output), s = f32(r*o), i0 = min(int(s), in-1),
    i1 = min(i0 + 1, in - 1), lambda = s - i0"""
    f = np.float32
    r = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0.0)
    s = (f(r) * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = (s - i0.astype(np.float32)).astype(np.float64)
    return i0, i1, lam


def bilinear_matrix(n_in, n_out):
    """dense interpolation matrix A [out, in]: out = A @ in along one axis"""
    i0, i1, lam = bilinear_taps(n_in, n_out)
    A = np.zeros((n_out, n_in))
    np.add.at(A, (np.arange(n_out), i0), 1.0 - lam)
    np.add.at(A, (np.arange(n_out), i1), lam)
    return A


def bilinear_fwd(x, ho, wo):
    """returns (out, terms): terms = sum of |weight * tap| over the four taps"""
    x = _f64(x)
    Ay, Ax = bilinear_matrix(x.shape[1], ho), bilinear_matrix(x.shape[2], wo)
    out = np.einsum("oh,nhwc->nowc", Ay, x, optimize=True)
    out = np.einsum("pw,nowc->nopc", Ax, out, optimize=True)
    ax = np.abs(x)
    terms = np.einsum("oh,nhwc->nowc", np.abs(Ay), ax, optimize=True)
    terms = np.einsum("pw,nowc->nopc", np.abs(Ax), terms, optimize=True)
    return out, terms


def bilinear_bwd(dout, h, w):
    """the explicit transpose: dx = A^T dout; returns (dx, terms, count) with count = taps summed into each input"""
    d = _f64(dout)
    Ay, Ax = bilinear_matrix(h, d.shape[1]), bilinear_matrix(w, d.shape[2])
    dx = np.einsum("oh,nopc->nhpc", Ay, d, optimize=True)
    dx = np.einsum("pw,nhpc->nhwc", Ax, dx, optimize=True)
    terms = np.einsum("oh,nopc->nhpc", Ay, np.abs(d), optimize=True)
    terms = np.einsum("pw,nhpc->nhwc", Ax, terms, optimize=True)
    count = np.outer((Ay != 0).sum(0), (Ax != 0).sum(0))
    return dx, terms, count


# ---- depth-to-space / space-to-depth: in[n,h,w,(dy*s+dx)*cout+co] <-> out[n,h*s+dy,w*s+dx,co] ----
def depth_to_space(x, s, bias=None):
    x = np.asarray(x)
    n, h, w, cc = x.shape
    cout = cc // (s * s)
    out = x.reshape(n, h, w, s, s, cout).transpose(0, 1, 3, 2, 4, 5).reshape(n, h * s, w * s, cout)
    return out if bias is None else _f64(out) + _f64(bias)


def space_to_depth(x, s):
    x = np.asarray(x)
    n, hs, ws, cout = x.shape
    return x.reshape(n, hs // s, s, ws // s, s, cout).transpose(0, 1, 3, 2, 4, 5).reshape(n, hs // s, ws // s, s * s * cout)


# ---- attention gate: out = x * p;  dx = dout * p, dp = sum_c dout * x ----
def gate_fwd(x, p):
    return _f64(x) * _f64(p)


def gate_bwd(dout, x, p):
    d, xx = _f64(dout), _f64(x)
    prod = d * xx
    return d * _f64(p), prod.sum(-1, keepdims=True), np.abs(prod).sum(-1, keepdims=True)


# ---- BatchNorm + PReLU: z = y*scale + shift; out = z > 0 ? z : alpha*z; dz = dout*(z > 0 ? 1 : alpha),
# ---- dalpha = sum dout * z * [z <= 0] (the slope branch at z == 0, as ATen) ----
def affine_prelu(y, scale, shift, alpha):
    ys = _f64(y) * _f64(scale)
    z = ys + _f64(shift)
    return np.where(z > 0, z, float(alpha) * z), np.abs(ys) + np.abs(_f64(shift)), z


def affine_prelu_bwd(dout, z, alpha):
    d, z = _f64(dout), _f64(z)
    neg = ~(z > 0)
    prod = np.where(neg, d * z, 0.0)
    return np.where(neg, d * float(alpha), d), prod.sum(), np.abs(prod).sum()


# ---- 1x1 convolution with K outputs: weight / bias gradients ----
def rowdot_bwd_weight(dy, x):
    """dy [npix, K], x [npix, c] -> (dw [K, c], db [K], |dw| terms, |db| terms)"""
    dy, x = _f64(dy), _f64(x)
    return dy.T @ x, dy.sum(0), np.abs(dy).T @ np.abs(x), np.abs(dy).sum(0)


def channel_sum(x):
    """x [..., c] -> (sum over everything but the channel, sum of |x|)"""
    x = _f64(x).reshape(-1, np.shape(x)[-1])
    return x.sum(0), np.abs(x).sum(0)
