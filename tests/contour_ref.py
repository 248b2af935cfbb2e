"""Integer / float64 numpy restatement of the contour metrics (oct_contour_update, evaluation.BoundaryEvaluator), the reference
the kernel and `evaluation.contour_metrics_from_records` are held to.

Contour points of a mask M: the midpoints of the in-image pairs of 4-adjacent pixels with exactly one pixel in M, in doubled
coordinates -- (2y, 2x+1) for the pair (y, x) | (y, x+1), (2y+1, 2x) for (y, x) | (y+1, x).  M_c = {label == c}; a pixel whose
target equals ignore_index is outside the image in both maps (a pair touching it yields no point).  Direction 0 goes from the
points of pred to the nearest point of target, direction 1 the reverse; D2 = the brute-force minimum of the squared distance
over ALL pairs, an exact integer (true distance sqrt(D2) / 2).

  records(...)      the five integers per (image, class, direction): n, max_d2, lo_d2, hi_d2, sum_q with
                    lo = 19 (n - 1) // 20, hi = min(lo + 1, n - 1), sum_q = sum math.isqrt(D2 << 32); zeros except n where a
                    side has no point
  float_metrics(...) an independent path: np.sqrt, np.max, np.percentile(., 95), np.mean on the same distance lists"""
import math

import numpy as np


def contour_points(mask, outside=None):
    """int64 [n, 2] doubled coordinates (Y, X) of the contour points of one H x W bool mask, rows first"""
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    out = np.zeros((h, w), dtype=bool) if outside is None else np.asarray(outside, dtype=bool)
    assert out.shape == (h, w)
    ys, xs = np.nonzero((m[:, :-1] != m[:, 1:]) & ~(out[:, :-1] | out[:, 1:]))     # (y, x) | (y, x + 1)
    yv, xv = np.nonzero((m[:-1, :] != m[1:, :]) & ~(out[:-1, :] | out[1:, :]))     # (y, x) | (y + 1, x)
    return np.concatenate([np.stack([2 * ys, 2 * xs + 1], axis=1), np.stack([2 * yv + 1, 2 * xv], axis=1)]).astype(np.int64)


def nearest_d2(src, dst):
    """int64 [len(src)]: min over dst of the squared distance, all pairs, as |s|^2 + min_d (|d|^2 - 2 s.d).  Every term is an
    integer: below 2^24 in float32 while the coordinates stay below 2^11, below 2^33 in float64 (coordinates below 2^15), so
    the arithmetic is exact"""
    ft = np.float32 if max(int(src.max()), int(dst.max())) < 2048 else np.float64
    s, d = src.astype(ft), dst.astype(ft)
    d_sq = (d * d).sum(axis=1)
    res = np.empty(len(src), dtype=np.int64)
    block = max(1, (1 << 23) // max(len(dst), 1))       # the pair matrix in slabs of at most 64 MiB
    for lo in range(0, len(src), block):
        a = s[lo:lo + block]
        m = (-2 * a) @ d.T
        m += d_sq[None, :]
        res[lo:lo + block] = (m.min(axis=1) + (a * a).sum(axis=1)).astype(np.int64)
    return res


def _distance_lists(target, pred, classes, ignore_index):
    """per image and class: (D2 of pred's points against target's, D2 of target's against pred's, n_pred, n_target)"""
    t = np.asarray(target).astype(np.int64)
    p = np.asarray(pred).astype(np.int64)
    assert t.shape == p.shape and t.ndim >= 2
    h, w = t.shape[-2:]
    t, p = t.reshape(-1, h, w), p.reshape(-1, h, w)
    res = []
    for ti, pi in zip(t, p):
        outside = (ti == ignore_index) if ignore_index is not None else np.zeros((h, w), dtype=bool)
        row = []
        for c in range(classes):
            pt, pp = contour_points(ti == c, outside), contour_points(pi == c, outside)
            if len(pt) and len(pp):
                row.append((nearest_d2(pp, pt), nearest_d2(pt, pp), len(pp), len(pt)))
            else:
                row.append((np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), len(pp), len(pt)))
        res.append(row)
    return res


def records_from_lists(lists):
    rec = np.zeros((len(lists), len(lists[0]) if lists else 0, 2, 5), dtype=np.int64)
    for i, row in enumerate(lists):
        for c, (d0, d1, n0, n1) in enumerate(row):
            for k, (d, n) in enumerate(((d0, n0), (d1, n1))):
                rec[i, c, k, 0] = n
                if len(d):
                    assert len(d) == n
                    s = np.sort(d)
                    lo = (19 * (n - 1)) // 20
                    hi = min(lo + 1, n - 1)
                    rec[i, c, k, 1:] = [s[-1], s[lo], s[hi], sum(math.isqrt(int(v) << 32) for v in d)]
    return rec


def records(target, pred, classes, ignore_index=None):
    """int64 [images, classes, 2, 5] of class maps (..., H, W)"""
    return records_from_lists(_distance_lists(target, pred, classes, ignore_index))


def float_metrics(target, pred, classes, ignore_index=None):
    """(hausdorff, hd95, assd), float64 [images, classes] each, NaN where a side has no point: np.sqrt / np.percentile / mean"""
    lists = _distance_lists(target, pred, classes, ignore_index)
    out = np.full((3, len(lists), classes), np.nan)
    for i, row in enumerate(lists):
        for c, (d0, d1, n0, n1) in enumerate(row):
            if n0 and n1:
                e0, e1 = np.sqrt(d0.astype(np.float64)) / 2.0, np.sqrt(d1.astype(np.float64)) / 2.0
                out[0, i, c] = max(e0.max(), e1.max())
                out[1, i, c] = max(np.percentile(e0, 95), np.percentile(e1, 95))
                out[2, i, c] = (e0.mean() + e1.mean()) / 2.0
    return out[0], out[1], out[2]


# ---- the known answers of the issue ---------------------------------------------------------------------------------------
def two_pixels():
    """8 x 10, single pixels at (3, 3) and (3, 6): HD 3.0, 4 points per side"""
    t, p = np.zeros((8, 10), dtype=np.uint8), np.zeros((8, 10), dtype=np.uint8)
    t[3, 3] = 1
    p[3, 6] = 1
    return t, p


def two_rectangles():
    """8 x 12, rectangles [2:5, 2:6] and [2:5, 4:8]: HD = HD95 = 2.0, 14 points per side"""
    t, p = np.zeros((8, 12), dtype=np.uint8), np.zeros((8, 12), dtype=np.uint8)
    t[2:5, 2:6] = 1
    p[2:5, 4:8] = 1
    return t, p


KNOWN = {   # name -> (maker, HD, HD95, ASSD, points per side)
    "two_pixels": (two_pixels, 3.0, 2.932426463519459, 2.524754878398196, 4),
    "two_rectangles": (two_rectangles, 2.0, 2.0, 0.9694174010713399, 14),
}


def mask_records(y_true, y_pred):
    """records [1, 1, 2, 5] of a pair of 0/1 masks: class 0 of the inverted masks, as Metrics.Contour_based_metrics runs them"""
    return records(1 - np.asarray(y_true, dtype=np.int64)[None], 1 - np.asarray(y_pred, dtype=np.int64)[None], 1)
