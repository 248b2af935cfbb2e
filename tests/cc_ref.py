"""Pure-numpy restatement of the connected-component entry points (include/oct_hip.h, "Connected components"): roots, info,
the cleanup filter and the lesion-wise counts.  tests/test_components_cpu.py checks it against scipy.ndimage.label.

Labelling: every inside pixel starts as its own index y*w + x; a sweep takes the minimum over the connected neighbours and then
follows the labels as pointers (L = L[L]) until nothing moves.  A label is always the index of a pixel of the same component
that is not larger than the pixel's own, so the fixed point is the component's smallest index.  The pointer jumps keep the
number of sweeps logarithmic on serpentines and spirals."""
import numpy as np

BORDER_BIT = 30


def inside(m, classes, ignore_index=None):
    m = np.asarray(m).astype(np.int64)
    ok = (m >= 0) & (m < classes)
    if ignore_index is not None:
        ok &= m != ignore_index
    return ok


def _classes_of(m, classes, ignore_index, outside=None):
    """int64 class per pixel, -1 outside"""
    m = np.asarray(m).astype(np.int64)
    ok = inside(m, classes, ignore_index)
    if outside is not None:
        ok &= ~outside
    return np.where(ok, m, -1)


def _label_image(cls, connectivity):
    """roots of one [h, w] image of classes (-1 outside)"""
    h, w = cls.shape
    n = h * w
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    big = np.int64(n)
    L = np.where(cls >= 0, idx, big)
    offs = [(0, 1), (1, 0)] if connectivity == 4 else [(0, 1), (1, 0), (1, 1), (1, -1)]
    pairs = []
    for dy, dx in offs:   # the slices of a pixel and of its neighbour at (dy, dx), both ways
        ya, yb = slice(0, h - dy), slice(dy, h)
        xa, xb = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
        same = (cls[ya, xa] == cls[yb, xb]) & (cls[ya, xa] >= 0)
        pairs.append(((ya, xa), (yb, xb), same))
    while True:
        before = L
        L = L.copy()
        for a, b, same in pairs:
            m = np.minimum(L[a], L[b])
            L[a] = np.where(same, np.minimum(L[a], m), L[a])   # a pixel is in both slices: never raise what the first wrote
            L[b] = np.where(same, np.minimum(L[b], m), L[b])
        flat = np.append(L.reshape(-1), big)   # the sentinel points at itself
        for _ in range(64):
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        L = flat[:n].reshape(h, w)
        if np.array_equal(L, before):
            break
    return np.where(cls >= 0, L, -1).astype(np.int32)


def _info_image(roots):
    h, w = roots.shape
    info = np.zeros(h * w, dtype=np.int64)
    flat = roots.reshape(-1)
    ok = flat >= 0
    np.add.at(info, flat[ok], 1)
    edge = np.zeros((h, w), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    touch = np.unique(flat[ok & edge.reshape(-1)])
    info[touch] |= 1 << BORDER_BIT
    return info.reshape(h, w).astype(np.int32)


def label(m, classes, connectivity=4, ignore_index=None, outside=None):
    """(roots, info) int32 of the map's shape; every leading dimension counts images"""
    m = np.asarray(m)
    h, w = m.shape[-2:]
    cls = _classes_of(m, classes, ignore_index, outside).reshape(-1, h, w)
    roots = np.stack([_label_image(c, connectivity) for c in cls]) if len(cls) else np.zeros((0, h, w), np.int32)
    info = np.stack([_info_image(r) for r in roots]) if len(cls) else np.zeros((0, h, w), np.int32)
    return roots.reshape(m.shape), info.reshape(m.shape)


def table(m, classes, connectivity=4, ignore_index=None):
    """int64 [n, 6]: image, class, root_y, root_x, area, touches_border, sorted by image, class, root"""
    m = np.asarray(m)
    h, w = m.shape[-2:]
    _, info = label(m, classes, connectivity, ignore_index)
    info = info.reshape(-1, h, w)
    mm = m.reshape(-1, h, w).astype(np.int64)
    rows = []
    for b, y, x in zip(*np.nonzero(info)):
        v = int(info[b, y, x])
        rows.append((b, int(mm[b, y, x]), y, x, v & ((1 << BORDER_BIT) - 1), v >> BORDER_BIT))
    rows.sort(key=lambda r: (r[0], r[1], r[2] * w + r[3]))
    return np.array(rows, dtype=np.int64).reshape(-1, 6)


def _per_class(v, classes):
    if v is None:
        return [0] * classes
    if np.isscalar(v) or isinstance(v, bool):
        return [int(v)] * classes
    v = [int(q) for q in v]
    assert len(v) == classes
    return v


def filter_map(m, classes, min_area=None, keep_largest=None, fill_enclosed=None, replace=0, connectivity=4, ignore_index=None):
    """one pass over the components of the input: the rules of oct_cc_filter"""
    m = np.asarray(m)
    h, w = m.shape[-2:]
    min_area, keep, drop, repl = (_per_class(v, classes) for v in (min_area, keep_largest, fill_enclosed, replace))
    roots, info = label(m, classes, connectivity, ignore_index)
    roots, info = roots.reshape(-1, h, w), info.reshape(-1, h, w)
    src = m.reshape(-1, h, w)
    out = src.copy()
    for b in range(len(src)):
        comps = {}
        for y, x in zip(*np.nonzero(info[b])):
            v = int(info[b, y, x])
            comps.setdefault(int(src[b, y, x]), []).append((int(y) * w + int(x), v & ((1 << BORDER_BIT) - 1), v >> BORDER_BIT))
        gone = np.zeros(h * w + 1, dtype=bool)           # by root; the last entry serves the outside pixels (root -1)
        for c, lst in comps.items():
            best = max(lst, key=lambda t: (t[1], -t[0]))[0]   # greatest area, ties to the smallest root
            for root, area, touches in lst:
                gone[root] = area < min_area[c] or (keep[c] and root != best) or (drop[c] and not touches)
        hit = gone[roots[b]]
        value = np.asarray(repl, dtype=np.int64)[np.where(hit, src[b], 0).astype(np.int64)]
        out[b] = np.where(hit, value.astype(src.dtype), src[b])
    return out.reshape(m.shape)


def lesion_state(target, pred, classes, connectivity=4, ignore_index=None, min_overlap=(0, 1)):
    """int64 [classes*4 + 4]: per class target components, predicted components, detected, confirmed; then images, ignored,
    invalid, updates -- one update of oct_lesion_eval_update on a zeroed state"""
    t, p = np.asarray(target).astype(np.int64), np.asarray(pred).astype(np.int64)
    assert t.shape == p.shape
    h, w = t.shape[-2:]
    num, den = min_overlap
    ign = (t == ignore_index) if ignore_index is not None else np.zeros(t.shape, dtype=bool)
    ct, cp = _classes_of(t, classes, None, ign), _classes_of(p, classes, None, ign)
    rt, it = label(t, classes, connectivity, None, ign)
    rp, ip = label(p, classes, connectivity, None, ign)
    state = np.zeros(classes * 4 + 4, dtype=np.int64)
    both = (ct == cp) & (ct >= 0)
    for cls, roots, info, col in ((ct, rt, it, 0), (cp, rp, ip, 1)):
        cls, roots, info, agree = (a.reshape(-1, h, w) for a in (cls, roots, info, both))
        for b in range(len(cls)):
            inter = np.zeros(h * w, dtype=np.int64)
            np.add.at(inter, roots[b][agree[b]], 1)
            for y, x in zip(*np.nonzero(info[b])):
                c = int(cls[b, y, x])
                area = int(info[b, y, x]) & ((1 << BORDER_BIT) - 1)
                n = int(inter[y * w + x])
                state[c * 4 + col] += 1
                if n >= 1 and n * den >= num * area:
                    state[c * 4 + 2 + col] += 1
    images = t.size // (h * w)
    state[classes * 4:] = (images, int(ign.sum()), int((~ign & ((ct < 0) | (cp < 0))).sum()), 1)
    return state


# ---- patterns ---------------------------------------------------------------------------------------------------------------
def serpentine(h, w):
    """class 1: full rows 0, 2, 4, ... joined at alternating ends -- one component that crosses every tile border many times"""
    m = np.zeros((h, w), dtype=np.int64)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, (w - 1) if k % 2 == 0 else 0] = 1
    return m


def spiral(h, w):
    """class 1: a path that winds inward with one-pixel walls and one-pixel gaps -- one component"""
    m = np.zeros((h, w), dtype=np.int64)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1

    def free(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or m[yy, xx] == 0

    while True:
        for _ in range(2):   # straight on while the cell ahead and the one behind it are free, else one turn to the right
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and m[ny, nx] == 0 and free(ny + dy, nx + dx):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return m
