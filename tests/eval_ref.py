"""int64 / float64 numpy restatement of the streaming segmentation evaluator (oct_seg_eval_update), the reference the kernel
and `evaluation.metrics_from_state` are held to.  Per pixel with target t and prediction p, C classes:

  ignored = ignore_index is given and t == ignore_index            -> state.ignored, nothing else
  invalid = not ignored and (t or p outside [0, C))                  -> state.invalid, nothing else
  valid   = every other pixel                                        -> cm[t][p] += 1
  thick_abs[c] += sum over images b and columns x of |T - P|,  T = #{y : valid, t == c},  P = #{y : valid, p == c}
  columns += images * W,  updates += 1
State layout: cm [C*C] | thick_abs [C] | columns | ignored | invalid | updates.  Everything is an integer: comparisons with the
kernel are exact.  `thickness_difference` restates Metrics/Biomarker_based_metrics.py:3-21 of the reference on one mask pair."""
import numpy as np


def state_size(classes):
    return classes * classes + classes + 4


def eval_state(target, pred, classes, ignore_index=None):
    """int64 state of ONE update with class maps (..., H, W)"""
    t = np.asarray(target).astype(np.int64)
    p = np.asarray(pred).astype(np.int64)
    assert t.shape == p.shape and t.ndim >= 2
    h, w = t.shape[-2:]
    t, p = t.reshape(-1, h, w), p.reshape(-1, h, w)
    ignored = (t == ignore_index) if ignore_index is not None else np.zeros(t.shape, dtype=bool)
    inrange = (t >= 0) & (t < classes) & (p >= 0) & (p < classes)
    valid = ~ignored & inrange
    state = np.zeros(state_size(classes), dtype=np.int64)
    cc = classes * classes
    state[:cc] = np.bincount((t[valid] * classes + p[valid]).ravel(), minlength=cc)
    for c in range(classes):
        tc = (valid & (t == c)).sum(axis=1, dtype=np.int64)     # [images, W]: thickness along H
        pc = (valid & (p == c)).sum(axis=1, dtype=np.int64)
        state[cc + c] = np.abs(tc - pc).sum()
    state[cc + classes:] = [t.shape[0] * w, ignored.sum(), (~ignored & ~inrange).sum(), 1]
    return state


def argmax_first(logits, axis):
    """first maximum wins, the first NaN beats everything (torch.argmax, numpy.argmax)"""
    return np.argmax(np.asarray(logits, dtype=np.float64), axis=axis).astype(np.int64)


def thickness_difference(y_true, y_pred):
    """the reference's thickness_difference on an H x W pair of bool masks (numpy sums bool in int64)"""
    a = np.sum(np.asarray(y_true), axis=0)
    b = np.sum(np.asarray(y_pred), axis=0)
    return np.mean(np.abs(a - b))


def one_vs_rest_counts(cm):
    """[C, 6] = tp, t, p, tn, fp, fn of every class from a confusion matrix"""
    cm = np.asarray(cm, dtype=np.int64)
    n, t, p, tp = cm.sum(), cm.sum(axis=1), cm.sum(axis=0), np.diagonal(cm)
    return np.stack([tp, t, p, n - t - p + tp, p - tp, t - tp], axis=1)


# ---- seeded class maps ----------------------------------------------------------------------------------------------------
def layered_maps(rng, shape, classes, jitter=2):
    """piecewise-constant "retinal layer" maps: per column, C bands along H with smoothly varying boundaries; the prediction
    moves every boundary by up to `jitter` rows"""
    h, w = shape[-2:]
    n = int(np.prod(shape[:-2], dtype=np.int64))
    yy = np.arange(h)[None, :, None]

    def bands(bounds):   # bounds [n, C-1, w] -> label = number of boundaries at or above the row
        lab = np.zeros((n, h, w), dtype=np.int64)
        for k in range(bounds.shape[1]):
            lab += yy >= bounds[:, k][:, None, :]
        return lab

    base = np.sort(rng.integers(0, h + 1, size=(n, max(classes - 1, 0), 1)), axis=1)
    wav = np.round(2.0 * np.sin(np.arange(w)[None, None, :] / 7.0 + rng.random((n, max(classes - 1, 0), 1)) * 6.0)).astype(np.int64)
    bt = np.sort(base + wav, axis=1)
    bp = np.sort(bt + rng.integers(-jitter, jitter + 1, size=bt.shape), axis=1)
    return bands(bt).reshape(shape), bands(bp).reshape(shape)


def random_maps(rng, shape, classes):
    return rng.integers(0, classes, size=shape), rng.integers(0, classes, size=shape)
