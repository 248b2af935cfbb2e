"""numpy restatement of the layer-surface definition (surfaces.py doc-string, include/oct_hip.h), with the recurrence written
literally.  The reference project has nothing to compare with, so test_surfaces_cpu.py pins this file against a brute force over
all paths; the GPU results are then pinned to it with ==."""
import numpy as np

BIG = np.iinfo(np.int64).max


def unary_map(m, order, classes, ignore_index=None):
    """int64 [K, H, W]: 0 where the pixel is free or its class is order[j], else 1"""
    m = np.asarray(m).astype(np.int64)
    free = ~np.isin(m, list(order)) | (m < 0) | (m >= classes)
    if ignore_index is not None:
        free |= m == ignore_index
    return np.stack([np.where(free | (m == c), 0, 1) for c in order]).astype(np.int64)


def unary_scores(z, order, scale=16.0, qmax=255):
    """int64 [K, H, W] of fp32 scores [C, H, W] (bf16 widened by the caller): every operation its own fp32 rounding"""
    z = np.asarray(z, dtype=np.float32)
    free = np.isnan(z).any(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(free, np.float32(0), np.fmax.reduce(z, axis=0)).astype(np.float32)
        out = []
        for c in order:
            zc = z[c]
            diff = np.where(zc == m, np.float32(0), (m - zc).astype(np.float32)).astype(np.float32)
            v = ((diff * np.float32(scale)).astype(np.float32) + np.float32(0.5)).astype(np.float32)
            u = np.where(v < np.float32(qmax + 1), np.floor(v), np.float32(qmax))
            out.append(np.where(free, 0, u).astype(np.int64))
    return np.stack(out)


def path_costs(u):
    """int64 [K-1, W, H+1]: N_k(x, s) = sum_{y<s} d_k(y, x), d_k = min_{j<k} u_j - min_{j>=k} u_j"""
    K, H, W = u.shape
    N = np.zeros((K - 1, W, H + 1), dtype=np.int64)
    for k in range(1, K):
        d = u[:k].min(axis=0) - u[k:].min(axis=0)                     # [H, W]
        N[k - 1, :, 1:] = np.cumsum(d, axis=0).T
    return N


def shortest_paths(N, max_step):
    """(paths int64 [..., W], costs int64 [...]): one path through every N [..., W, H+1] by the recurrence of the definition
    (the leading dimensions are independent problems solved side by side)"""
    W, S = N.shape[-2:]
    if max_step is None:
        s = N.argmin(axis=-1)                                         # numpy's argmin is the smallest
        return s.astype(np.int64), np.take_along_axis(N, s[..., None], axis=-1)[..., 0].sum(axis=-1)
    A = N[..., 0, :].copy()                                           # A(0, s) = N(0, s)
    P = np.zeros(N.shape, dtype=np.int64)
    for x in range(1, W):
        best = np.full(A.shape, BIG, dtype=np.int64)
        bt = np.full(A.shape, -1, dtype=np.int64)
        for off in range(-max_step, max_step + 1):                    # t = s + off ascending, strict <: the smallest t stays
            lo, hi = max(0, -off), min(S, S - off)                    # the s whose t lies in 0..H
            if lo >= hi:
                continue
            cand = A[..., lo + off:hi + off]
            take = cand < best[..., lo:hi]
            best[..., lo:hi] = np.where(take, cand, best[..., lo:hi])
            bt[..., lo:hi] = np.where(take, np.arange(lo + off, hi + off), bt[..., lo:hi])
        P[..., x, :] = bt
        A = N[..., x, :] + best
    path = np.zeros(N.shape[:-1], dtype=np.int64)
    path[..., W - 1] = A.argmin(axis=-1)                              # the smallest argmin of the last column
    for x in range(W - 1, 0, -1):
        path[..., x - 1] = np.take_along_axis(P[..., x, :], path[..., x, None], axis=-1)[..., 0]
    return path, A.min(axis=-1)


def shortest_path(N, max_step):
    """(path int64 [W], its cost) of one surface through N [W, H+1]"""
    path, cost = shortest_paths(N, max_step)
    return path, int(cost)


def surfaces_from_unary(u, max_step, raw=False):
    """int32 [K-1, W]; raw=True: before s_k <- max(s_k, s_{k-1})"""
    s = shortest_paths(path_costs(u), max_step)[0]
    if not raw:
        s = np.maximum.accumulate(s, axis=0)
    return s.astype(np.int32)


def extract(maps, order, classes, max_step=1, ignore_index=None):
    """int32 (*lead, K-1, W) of integer class maps (*lead, H, W)"""
    maps = np.asarray(maps)
    h, w = maps.shape[-2:]
    flat = maps.reshape(-1, h, w)
    out = [surfaces_from_unary(unary_map(m, order, classes, ignore_index), max_step) for m in flat]
    return np.stack(out).reshape(maps.shape[:-2] + (len(order) - 1, w)) if out else np.zeros(maps.shape[:-2] + (len(order) - 1, w), np.int32)


def extract_scores(z, order, max_step=1, scale=16.0, qmax=255):
    """int32 (B, K-1, W) of fp32 scores (B, C, H, W)"""
    return np.stack([surfaces_from_unary(unary_scores(zi, order, scale, qmax), max_step) for zi in z])


def argmax_first(z):
    """the package's arg-max over axis 0 of [C, H, W]: first maximum wins, the first NaN beats everything"""
    z = np.asarray(z, dtype=np.float32)
    best, arg = z[0].copy(), np.zeros(z.shape[1:], dtype=np.int64)
    for c in range(1, z.shape[0]):
        with np.errstate(invalid="ignore"):
            take = (z[c] > best) | (np.isnan(z[c]) & ~np.isnan(best))
        best = np.where(take, z[c], best)
        arg = np.where(take, c, arg)
    return arg


def paint(surfaces, order, h, keep=(), input_classes=None):
    """int64 (*lead, H, W): out(y, x) = order[#{k : s_k(x) <= y}]; input_classes (*lead, H, W) kept where listed in keep"""
    s = np.asarray(surfaces).astype(np.int64)
    y = np.arange(h).reshape((1,) * (s.ndim - 2) + (1, h, 1))
    count = (s[..., :, None, :] <= y).sum(axis=-3)
    out = np.asarray(order, dtype=np.int64)[count]
    if len(keep):
        cls = np.asarray(input_classes).astype(np.int64)
        out = np.where(np.isin(cls, list(keep)), cls, out)
    return out


def error_state(target, pred, valid=None):
    """int64 [K-1, 5]: count, sum |e|, sum e, sum e^2, max |e| over the valid columns; surfaces (*lead, K-1, W)"""
    t, p = np.asarray(target).astype(np.int64), np.asarray(pred).astype(np.int64)
    k, w = t.shape[-2:]
    e = (p - t).reshape(-1, k, w)
    ok = np.ones((e.shape[0], w), dtype=bool) if valid is None else np.asarray(valid).astype(bool).reshape(-1, w)
    st = np.zeros((k, 5), dtype=np.int64)
    for i in range(k):
        v = e[:, i][ok]
        st[i] = (v.size, np.abs(v).sum(), v.sum(), (v * v).sum(), np.abs(v).max() if v.size else 0)
    return st


def band_map(h, w, cuts):
    """a valid band map: cuts int [K-1, W] non-decreasing down the surfaces; class j between cut j-1 and cut j"""
    y = np.arange(h)[:, None]
    return (np.asarray(cuts)[:, None, :] <= y[None]).sum(axis=0).astype(np.int64)
