"""int64 numpy restatement of the score evaluator (oct_score_eval_update), the reference the kernel and
`evaluation.score_metrics_from_state` are held to.

The key.  key16(v) of a non-NaN float32 v is the order-preserving code of v rounded toward -inf onto the bf16 grid:
  u = bits(v), h = u >> 16, low = u & 0xFFFF
  sign clear:  key = 0x8000 + h
  sign set:    m = (h & 0x7FFF) + (low != 0), capped at 0x7F80;  key = 0x8000 - m
-0.0 and +0.0 share key 0x8000; keys lie in [0x0080, 0xFF80]; bin k is the half-open interval [g(k), g(k+1)) of the real line,
so for a threshold theta on the bf16 grid v >= theta <=> key16(v) >= key16(theta) for every fp32 v, negative theta included.

State layout, C channels: hist[C][2][65536] | nan[C] | ignored[C] | invalid[C] | updates.  Per element of channel c with target
t and score v, decided in this order:
  ignore_value is given and t == ignore_value  -> ignored[c]
  t > 1                                        -> invalid[c]
  v is NaN                                     -> nan[c]
  otherwise                                    -> hist[c][t][key16(v)]
updates += 1 per call.  Everything is an integer: comparisons with the kernel are exact."""
import numpy as np

KEYS = 65536
# bf16 grid points, each also one float32 ulp above and below in the tests
GRID = (-2.0, -1.0, -2.0 ** -7, 0.0, 2.0 ** -7, 1.0, 2.0)


def state_size(channels):
    return channels * (2 * KEYS + 3) + 1


def key16(v):
    """by float32 bit operations; any shape, no NaN"""
    a = np.asarray(v, dtype=np.float32)
    u = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.int64).reshape(a.shape)
    h, low = u >> 16, u & 0xFFFF
    neg = (u >> 31) == 1
    m = np.minimum((h & 0x7FFF) + (low != 0).astype(np.int64), 0x7F80)
    return np.where(neg, 0x8000 - m, 0x8000 + h)


def score_state(target, scores, channels, ignore_value=None):
    """int64 state of ONE update: target uint8 and scores (float32 values) of shape [images, channels, h, w]"""
    t = np.asarray(target).astype(np.int64)
    v = np.asarray(scores, dtype=np.float32)
    assert t.shape == v.shape and t.ndim == 4 and t.shape[1] == channels
    state = np.zeros(state_size(channels), dtype=np.int64)
    hist = state[:channels * 2 * KEYS].reshape(channels, 2, KEYS)
    tail = state[channels * 2 * KEYS:]
    for c in range(channels):
        tc, vc = t[:, c].ravel(), v[:, c].ravel()
        ignored = (tc == ignore_value) if ignore_value is not None else np.zeros(tc.shape, dtype=bool)
        invalid = ~ignored & (tc > 1)
        isnan = ~ignored & ~invalid & np.isnan(vc)
        ok = ~ignored & ~invalid & ~isnan
        k = key16(np.where(ok, vc, np.float32(0)))
        hist[c] = np.bincount((tc[ok] * KEYS + k[ok]), minlength=2 * KEYS).reshape(2, KEYS)
        tail[c], tail[channels + c], tail[2 * channels + c] = isnan.sum(), ignored.sum(), invalid.sum()
    tail[3 * channels] = 1
    return state


def ulp_neighbours(values):
    """every value with the float32 one ulp below and above it"""
    g = np.asarray(values, dtype=np.float32)
    return np.concatenate([np.nextafter(g, np.float32(-np.inf)), g, np.nextafter(g, np.float32(np.inf))]).astype(np.float32)


def special_values():
    """+-0, +-inf, denormals, +-max and the grid points with their float32 neighbours"""
    fi = np.finfo(np.float32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, -fi.tiny / 2,
                   fi.tiny, -fi.tiny, fi.max, -fi.max], dtype=np.float32)
    return np.concatenate([sp, ulp_neighbours(GRID)])


# ---- seeded fields: (target uint8, scores float32) of shape [images, channels, h, w] -----------------------------------------
def _labels(rng, shape, scores):
    """a label that follows the score, with noise: both labels appear wherever there is more than a handful of elements"""
    return ((scores + rng.standard_normal(shape).astype(np.float32)) > 0.5).astype(np.uint8)


def smooth_field(rng, shape):
    """what logits look like: a few smooth blobs on a negative background, so neighbouring pixels share keys"""
    n, c, h, w = shape
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    s = np.full(shape, -4.0, dtype=np.float32)
    for i in range(n):
        for j in range(c):
            for _ in range(2):
                cy, cx, r = rng.random() * h, rng.random() * w, 1.0 + rng.random() * max(h, w) / 3
                s[i, j] += (8.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))).astype(np.float32)
    return _labels(rng, shape, s), s


def random_field(rng, shape):
    """i.i.d. N(0, 3) fp32: up to 64 distinct keys per wave"""
    s = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    return _labels(rng, shape, s), s


def constant_field(shape, value=-3.0, label=0):
    """one key and one label everywhere: the maximum-conflict case"""
    return np.full(shape, label, dtype=np.uint8), np.full(shape, value, dtype=np.float32)


def special_field(rng, shape):
    """the special values and grid neighbours, plus NaNs, drawn at random over the field"""
    pool = np.concatenate([special_values(), np.array([np.nan, -np.nan], dtype=np.float32)])
    s = pool[rng.integers(0, pool.size, size=shape)].astype(np.float32)
    return rng.integers(0, 2, size=shape).astype(np.uint8), s


def to_bf16_values(scores):
    """float32 values rounded to nearest-even onto the bf16 grid (NaN stays NaN): what a bf16 tensor of them holds"""
    a = np.asarray(scores, dtype=np.float32)
    u = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = np.where(np.isnan(a.reshape(-1)), np.uint64(0x7FC00000), r).astype(np.uint32).view(np.float32)
    return out.reshape(a.shape)
