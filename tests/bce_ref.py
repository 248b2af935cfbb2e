"""Float64 numpy restatement of the binary / multi-label loss head (sigmoid BCE + soft Dice), the reference the oct_bce_loss_*
kernels are held to.  Per element: logit x at (image, channel c, pixel i), target t a uint8 mask value.

  valid = not (ignore_value is given and t == ignore_value)
  omega = valid * pixel_weight[image, i]                       (1 without a map; one value for all channels of a pixel)
  l     = (1 - t) x + (1 + (pos_weight[c] - 1) t) (log1p(exp(-|x|)) + max(-x, 0))      NaN for a valid t outside {0, 1}
  BCE   = sum omega l / sum omega                              (everything ignored: 0 / 0 = NaN)
  I_c, P_c, Y_c = sum s t, sum s, sum t over the valid elements of channel c, s = sigmoid(x), not weighted by the map
  Dice  = 1 - mean_c (2 I_c + eps) / (P_c + Y_c + eps);   loss = w_bce BCE + w_dice Dice
  dx    = g [w_bce (omega / sum omega) (s (1 - t + pos_weight t) - pos_weight t) + s (1 - s) (A_c t + B_c)], 0 where ignored
          A_c = -w_dice / C * 2 / den_c,  B_c = w_dice / C * num_c / den_c^2,  num_c = 2 I_c + eps,  den_c = P_c + Y_c + eps
With w_dice == 0 the Dice entry is 0 (its sums are not accumulated).  tests/test_bce_loss_cpu.py holds this file to float64
torch autograd."""
import numpy as np


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _prepare(x, t, pos_weight, pixel_weight, ignore_value):
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t)
    b, c, h, w = x.shape
    t = t.reshape(b, c, h, w).astype(np.int64)
    valid = np.ones(t.shape, dtype=bool) if ignore_value is None else t != ignore_value
    pw = np.ones(c) if pos_weight is None else np.asarray(pos_weight, dtype=np.float64)
    pm = np.ones((b, h, w)) if pixel_weight is None else np.asarray(pixel_weight, dtype=np.float64)
    omega = np.where(valid, np.broadcast_to(pm[:, None], t.shape), 0.0)
    tv = np.where(valid, t, 0).astype(np.float64)          # ignored elements enter through selects only
    xv = np.where(valid, x, 0.0)
    return xv, t, tv, valid, pw.reshape(1, c, 1, 1), omega


def forward(x, t, w_bce=1.0, w_dice=0.0, eps=1e-7, pos_weight=None, pixel_weight=None, ignore_value=None):
    """x: (B, C, H, W), t: uint8 (B, C, H, W) (or (B, H, W) for C == 1) -> ([loss, bce, dice] float64, cache)"""
    xv, t, tv, valid, pw, omega = _prepare(x, t, pos_weight, pixel_weight, ignore_value)
    c = xv.shape[1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        le = (1.0 - tv) * xv + (1.0 + (pw - 1.0) * tv) * (np.log1p(np.exp(-np.abs(xv))) + np.maximum(-xv, 0.0))
        le = np.where(valid & (t > 1), np.nan, le)
        wsum = omega.sum()
        bce = np.where(valid, omega * le, 0.0).sum() / wsum
    s = _sigmoid(xv)
    v = valid.astype(np.float64)
    if w_dice != 0.0:
        inter, ps, ys = (s * tv * v).sum((0, 2, 3)), (s * v).sum((0, 2, 3)), (tv * v).sum((0, 2, 3))
        num, den = 2.0 * inter + eps, ps + ys + eps
        dice = 1.0 - (num / den).mean()
    else:
        num, den, dice = np.full(c, eps), np.full(c, eps), 0.0
    loss = w_bce * bce + w_dice * dice
    return np.array([loss, bce, dice]), (s, tv, valid, pw, omega, wsum, num, den)


def backward(cache, w_bce=1.0, w_dice=0.0, g=1.0):
    """d(loss)/dx (B, C, H, W) float64 from forward()'s cache; g: the upstream gradient"""
    s, tv, valid, pw, omega, wsum, num, den = cache
    c = s.shape[1]
    a = (-w_dice / c * 2.0 / den).reshape(1, c, 1, 1)
    b = (w_dice / c * num / (den * den)).reshape(1, c, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = w_bce * (omega / wsum) * (s * (1.0 - tv + pw * tv) - pw * tv) + s * (1.0 - s) * (a * tv + b)
    return np.where(valid, g * d, 0.0)


def loss_and_grad(x, t, w_bce=1.0, w_dice=0.0, eps=1e-7, pos_weight=None, pixel_weight=None, ignore_value=None, g=1.0):
    out, cache = forward(x, t, w_bce, w_dice, eps, pos_weight, pixel_weight, ignore_value)
    return out, backward(cache, w_bce, w_dice, g)


def mask(x, tau):
    """uint8 (B, C, H, W) = x >= tau in the logits' own precision; a NaN logit gives 0"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return (x >= x.dtype.type(tau)).astype(np.uint8)


def threshold_to_tau(threshold):
    """float32(log(threshold / (1 - threshold)))"""
    return float(np.float32(np.log(threshold / (1.0 - threshold))))
