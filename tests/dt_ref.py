"""Pure-numpy restatement of the distance-map entry points (include/oct_hip.h, "Distance maps"): the valid mask, the three site
sets, the exact squared distance by the separable definition, the table lookup and the signed map in float64.
tests/test_distance_cpu.py checks it against scipy.ndimage.distance_transform_edt and against an all-pairs minimum.

Separable definition: g[y][x] = min over the sites (ys, x) of column x of |y - ys| (none: GFAR), then
    D2[y][x] = min over the columns x' with g[y][x'] != GFAR of (x - x')^2 + g[y][x']^2
which is the minimum of (y - ys)^2 + (x - xs)^2 over all sites with the minimum over ys taken first.  The minimum over x' is
taken literally, over the columns that can matter: column by column where few columns hold a site, offset by offset
r = |x - x'| = 0, 1, ... otherwise, ending once r^2 has reached the largest distance still standing (no later column can
lower any pixel then)."""
import numpy as np

FAR = 1 << 30
GFAR = 0xFFFF
_SPARSE_COLUMNS = 48


def valid(m, classes, ignore_index=None):
    m = np.asarray(m).astype(np.int64)
    ok = (m >= 0) & (m < classes)
    if ignore_index is not None:
        ok &= m != ignore_index
    return ok


def sites(m, classes, plane, ignore_index=None):
    """bool, the shape of m (..., h, w): the site set of "boundary", ("class", c) or ("other", c)"""
    m = np.asarray(m).astype(np.int64)
    ok = valid(m, classes, ignore_index)
    if plane == "boundary":
        out = np.zeros(m.shape, dtype=bool)
        h, w = m.shape[-2:]
        for axis, n in ((-2, h), (-1, w)):              # every in-image pair of 4-neighbours, both ways
            a = [slice(None)] * m.ndim
            b = [slice(None)] * m.ndim
            a[axis], b[axis] = slice(0, n - 1), slice(1, n)
            a, b = tuple(a), tuple(b)
            differ = ok[a] & ok[b] & (m[a] != m[b])
            out[a] |= differ
            out[b] |= differ
        return out
    kind, c = plane
    assert 0 <= c < classes
    if kind == "class":
        return ok & (m == c)
    assert kind == "other"
    return ok & (m != c)


def column_distance(s):
    """int64 [h, w]: the vertical distance to the nearest site of the column, GFAR where the column has none"""
    h, w = s.shape
    big = 4 * (h + 1)
    yy = np.arange(h, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(s, yy, -big), axis=0)             # the last site at or above
    below = np.minimum.accumulate(np.where(s, yy, big)[::-1], axis=0)[::-1]  # the first site at or below
    g = np.minimum(yy - above, below - yy)
    return np.where(g >= h, GFAR, g)


def row_minimum(g):
    """int64 [h, w]: min over x' of (x - x')^2 + g[y][x']^2 over the columns with a site, FAR where there is none"""
    h, w = g.shape
    have = g != GFAR
    best = np.full((h, w), FAR, dtype=np.int64)
    cols = np.flatnonzero(have.any(axis=0))               # a column with a site has one for every row
    if cols.size == 0:
        return best
    g2 = np.where(have, g * g, FAR)
    xx = np.arange(w, dtype=np.int64)[None, :]
    if cols.size <= _SPARSE_COLUMNS:
        for xs in cols:
            np.minimum(best, (xx - xs) ** 2 + g2[:, xs:xs + 1], out=best)
        return best
    for r in range(w):
        if r * r >= best.max():
            break
        np.minimum(best[:, r:], g2[:, :w - r] + r * r, out=best[:, r:])      # the column r to the left
        np.minimum(best[:, :w - r], g2[:, r:] + r * r, out=best[:, :w - r])  # the column r to the right
    return best


def squared_image(s):
    """int64 [h, w]: the exact squared distance to the nearest True of s, FAR everywhere when s has none"""
    return row_minimum(column_distance(s))


def squared_distance(m, classes, planes, ignore_index=None):
    """int32 (*lead, P, h, w), as distance.squared_distance"""
    m = np.asarray(m).astype(np.int64)
    h, w = m.shape[-2:]
    flat = m.reshape(-1, h, w)
    out = np.empty((flat.shape[0], len(planes), h, w), dtype=np.int32)
    for p, plane in enumerate(planes):
        s = sites(flat, classes, plane, ignore_index)
        for i in range(flat.shape[0]):
            out[i, p] = squared_image(s[i])
    return out.reshape(m.shape[:-2] + (len(planes), h, w))


def table_lookup(d2, table):
    """table[min(D2, len - 1)], the table as it is (fp32 in, fp32 out)"""
    table = np.asarray(table)
    return table[np.minimum(np.asarray(d2).astype(np.int64), table.shape[0] - 1)]


def weight_map(m, classes, table, ignore_index=None):
    """the dtype of `table`, the shape of m: as distance.DistanceWeightMap"""
    d2 = squared_distance(m, classes, ["boundary"], ignore_index)
    return table_lookup(d2[..., 0, :, :], table)


def signed_distance(m, classes, class_ids=None, ignore_index=None):
    """float64 (*lead, K, h, w): -sqrt(D2 to the valid pixels of other classes) on a pixel of class c, +sqrt(D2 to class c) on
    every other pixel; the whole plane of an image 0 when either set is empty"""
    m = np.asarray(m).astype(np.int64)
    ids = list(range(classes)) if class_ids is None else list(class_ids)
    h, w = m.shape[-2:]
    flat = m.reshape(-1, h, w)
    out = np.zeros((flat.shape[0], len(ids), h, w), dtype=np.float64)
    for k, c in enumerate(ids):
        s_in = sites(flat, classes, ("class", c), ignore_index)
        s_out = sites(flat, classes, ("other", c), ignore_index)
        for i in range(flat.shape[0]):
            if not s_in[i].any() or not s_out[i].any():
                continue
            to_class = np.sqrt(squared_image(s_in[i]).astype(np.float64))
            to_other = np.sqrt(squared_image(s_out[i]).astype(np.float64))
            out[i, k] = np.where(s_in[i], -to_other, to_class)
    return out.reshape(m.shape[:-2] + (len(ids), h, w))


def brute_force(s):
    """int64 [h, w]: the all-pairs minimum, for small maps"""
    h, w = s.shape
    ys, xs = np.nonzero(s)
    if ys.size == 0:
        return np.full((h, w), FAR, dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
    return d.min(axis=-1).astype(np.int64)


def wavy_bands(rng, shape, classes=6):
    """what an OCT map looks like: `classes` horizontal bands whose boundaries wave along the columns, int64 (*lead, h, w)"""
    h, w = shape[-2:]
    n = int(np.prod(shape[:-2], dtype=np.int64))
    yy = np.arange(h)[None, :, None]
    base = np.sort(rng.integers(0, h + 1, size=(n, classes - 1, 1)), axis=1)
    wave = np.round(3.0 * np.sin(np.arange(w)[None, None, :] / 9.0 + rng.random((n, classes - 1, 1)) * 6.0)).astype(np.int64)
    bounds = np.sort(base + wave, axis=1)
    m = np.zeros((n, h, w), dtype=np.int64)
    for k in range(classes - 1):
        m += yy >= bounds[:, k][:, None, :]
    return m.reshape(shape)
