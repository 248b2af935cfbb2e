"""Numpy restatement of the paired augmentation (a helper, not a test).  Independent of the product's augment.py: int64
coordinates, float32 arithmetic with one operation per rounding, Philox4x32-10 on uint64, float64 noise and gamma.

    SX = a xo + b yo + c + DX,  SY = d xo + e yo + f + DY                     (Q24, int64)
    ix = SX >> 24, wx = ((SX >> 8) & 0xFFFF) 2^-16, nearest (SX + 2^23) >> 24
    image / weight: (1-wy)((1-wx) p00 + wx p01) + wy((1-wx) p10 + wx p11), outside taps read fill / 0
    labels: nearest, outside reads label_fill
    intensity: v gain + bias -> [gamma] -> [noise] -> clamp -> round
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(counter, key):
    """Philox4x32-10: counter (..., 4), key (k0, k1) -> uint32 (..., 4)"""
    c = [(np.asarray(counter, dtype=np.uint64)[..., i] & M32) for i in range(4)]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        prod0 = np.uint64(0xD2511F53) * c[0]
        prod1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(prod1 >> S32) ^ c[1] ^ k0, prod1 & M32, (prod0 >> S32) ^ c[3] ^ k1, prod0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def grid_shape(out_hw, pitch):
    return -(-(out_hw[0] - 1) // pitch) + 1, -(-(out_hw[1] - 1) // pitch) + 1


def displacement(nodes, out_hw, pitch):
    """integer bilinear blend of one int32 Q24 node plane (gh, gw) -> int64 (Ho, Wo)"""
    ho, wo = out_hw
    k = pitch.bit_length() - 1
    assert 1 << k == pitch
    n = nodes.astype(np.int64)
    gh, gw = n.shape
    assert (gh, gw) == grid_shape(out_hw, pitch)
    yo, xo = np.arange(ho, dtype=np.int64)[:, None], np.arange(wo, dtype=np.int64)[None, :]
    i, ry, j, rx = yo >> k, yo & (pitch - 1), xo >> k, xo & (pitch - 1)
    i1, j1 = np.minimum(i + 1, gh - 1), np.minimum(j + 1, gw - 1)   # past the grid only with weight 0
    top = n[i, j] * (pitch - rx) + n[i, j1] * rx
    bot = n[i1, j] * (pitch - rx) + n[i1, j1] * rx
    return (top * (pitch - ry) + bot * ry) >> (2 * k)


def coords(matrix, out_hw, disp=None, pitch=None):
    """matrix int64 (6,) a b c d e f; disp int32 (2, gh, gw) or None -> SX, SY int64 (Ho, Wo)"""
    a, b, c, d, e, f = (int(v) for v in matrix)
    yo, xo = np.arange(out_hw[0], dtype=np.int64)[:, None], np.arange(out_hw[1], dtype=np.int64)[None, :]
    sx, sy = a * xo + b * yo + c, d * xo + e * yo + f
    if disp is not None:
        sx, sy = sx + displacement(disp[0], out_hw, pitch), sy + displacement(disp[1], out_hw, pitch)
    return sx, sy


def _tap(plane, y, x, oob):
    hs, ws = plane.shape
    ok = (y >= 0) & (y < hs) & (x >= 0) & (x < ws)
    v = plane[np.clip(y, 0, hs - 1), np.clip(x, 0, ws - 1)].astype(np.float32)
    return np.where(ok, v, np.float32(oob)).astype(np.float32)


def bilinear(plane, sx, sy, oob):
    """float32, every multiply and add rounded on its own"""
    ix, iy = sx >> 24, sy >> 24
    wx = (((sx >> 8) & 0xFFFF).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
    wy = (((sy >> 8) & 0xFFFF).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)
    one = np.float32(1.0)
    p00, p01 = _tap(plane, iy, ix, oob), _tap(plane, iy, ix + 1, oob)
    p10, p11 = _tap(plane, iy + 1, ix, oob), _tap(plane, iy + 1, ix + 1, oob)
    top = ((one - wx) * p00).astype(np.float32) + (wx * p01).astype(np.float32)
    bot = ((one - wx) * p10).astype(np.float32) + (wx * p11).astype(np.float32)
    return (((one - wy) * top).astype(np.float32) + (wy * bot).astype(np.float32)).astype(np.float32)


def nearest(plane, sx, sy, fill):
    nx, ny = (sx + (1 << 23)) >> 24, (sy + (1 << 23)) >> 24
    hs, ws = plane.shape
    ok = (ny >= 0) & (ny < hs) & (nx >= 0) & (nx < ws)
    v = plane[np.clip(ny, 0, hs - 1), np.clip(nx, 0, ws - 1)]
    return np.where(ok, v, np.asarray(fill, dtype=plane.dtype))


def normals(out_hw, channel, sample, step, key):
    """z1, z2 float64 (Ho, Wo) of one plane: counter ((pixel >> 1), channel, sample, step); the even pixel of a pair takes
    words 0,1, the odd one words 2,3"""
    ho, wo = out_hw
    pix = np.arange(ho * wo, dtype=np.uint64)
    ctr = np.stack([pix >> np.uint64(1), np.full_like(pix, channel), np.full_like(pix, sample), np.full_like(pix, step)], axis=-1)
    w = philox(ctr, key)
    odd = (pix & np.uint64(1)).astype(bool)
    wa, wb = np.where(odd, w[:, 2], w[:, 0]), np.where(odd, w[:, 3], w[:, 1])
    u1 = ((wa >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (wb >> 9).astype(np.float64) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u1))
    return (r * np.cos(2.0 * np.pi * u2)).reshape(ho, wo), (r * np.sin(2.0 * np.pi * u2)).reshape(ho, wo)


def to_bf16_bits(v):
    """float32 -> bf16 bits (uint16), round to nearest even (no NaN in the tests)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def augment(src, matrix, out_hw, intensity=None, gamma=False, noise=False, disp=None, pitch=None, fill=0.0, target=None,
            mask=None, weight=None, label_fill=0, key=(0, 0), step=0, sample_base=0, out_bf16=False):
    """src (B, C, Hs, Ws) uint8 / float32 (bf16 sources come as the float32 of the same values); matrix int64 (B, 6); intensity
    float32 (B, 7) gain bias gamma sigma_speckle sigma_add out_lo out_hi.
    -> dict: image (float32, or bf16 bits with out_bf16), exact (float64: the image before the final rounding, with gamma and
    noise in float64), target int64, mask uint8, weight float32"""
    b, cin = src.shape[:2]
    ho, wo = out_hw
    if intensity is None:
        intensity = np.tile(np.array([1, 0, 1, 0, 0, -np.inf, np.inf], dtype=np.float32), (b, 1))
    intensity = np.asarray(intensity, dtype=np.float32)
    img = np.empty((b, cin, ho, wo), dtype=np.float32)
    exact = np.empty((b, cin, ho, wo), dtype=np.float64)
    t_out = np.empty((b, ho, wo), dtype=np.int64) if target is not None else None
    m_out = np.empty((b, mask.shape[1], ho, wo), dtype=np.uint8) if mask is not None else None
    w_out = np.empty((b, ho, wo), dtype=np.float32) if weight is not None else None
    for s in range(b):
        sx, sy = coords(matrix[s], out_hw, None if disp is None else disp[s], pitch)
        gain, bias, gam, s_sp, s_ad, lo, hi = (np.float32(v) for v in intensity[s])
        for c in range(cin):
            v = bilinear(src[s, c], sx, sy, fill)
            v = ((v * gain).astype(np.float32) + bias).astype(np.float32)
            e = v.astype(np.float64)
            if gamma:
                t = np.clip(e, 0.0, 1.0)
                e = np.where(t > 0, np.power(np.where(t > 0, t, 1.0), float(gam)), 0.0)
            if noise:
                z1, z2 = normals(out_hw, c, sample_base + s, step, key)
                e = e * (1.0 + float(s_sp) * z1) + float(s_ad) * z2
            e = np.minimum(np.maximum(e, float(lo)), float(hi))
            exact[s, c] = e
            img[s, c] = e.astype(np.float32)   # without gamma and noise e holds float32 values: this is exact
        if target is not None:
            t_out[s] = nearest(target[s].astype(np.int64), sx, sy, label_fill)
        if mask is not None:
            for c in range(mask.shape[1]):
                m_out[s, c] = nearest(mask[s, c], sx, sy, label_fill)
        if weight is not None:
            w_out[s] = bilinear(weight[s], sx, sy, 0.0)
    return {"image": to_bf16_bits(img) if out_bf16 else img, "exact": exact, "target": t_out, "mask": m_out, "weight": w_out}
