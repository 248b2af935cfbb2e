"""Exactly representable operands for the bit-equality tests of the bf16 kernels (tests/test_gpu_exact.py,
tests/test_gpu_tile_walk.py): small integers, signed powers of two, dyadic BatchNorm coefficients.  Every product is exact,
every partial sum a multiple of a known granule far below 2^24 of them, so fp32 accumulation in ANY order gives the float64
result and the only rounding left is the final bf16 store.  The host halves (`*_host`) need no GPU."""
import numpy as np
import torch


def to_bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def dev(a_nchw):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a_nchw, np.float32).transpose(0, 2, 3, 1))).to("cuda", torch.bfloat16)


def host(t_nhwc):
    return t_nhwc.float().cpu().numpy().transpose(0, 3, 1, 2)


def fdev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda().contiguous()


def ints(rng, shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def pow2_weights(rng, shape, density=0.6, kmin=-3):
    """0 or +-2^k, k in {kmin..0}"""
    mag = np.exp2(rng.integers(kmin, 1, shape)).astype(np.float32)
    sign = rng.choice([-1.0, 1.0], shape).astype(np.float32)
    keep = (rng.random(shape) < density).astype(np.float32)
    return mag * sign * keep


def exact_src_host(rng, n, h, w, c0, c1, xform):
    """integer sources; on-load transform max(x*s + b, 0) with s in {+-0.5, +-1, 2}, b in halves: exact in fp32 and
    exactly representable in bf16 (multiples of 0.5 below 16).
    -> (x0, (s0, b0) | None, x1 | None, (s1, b1) | None, the effective float64 input of the convolution)"""
    parts = []
    x0 = ints(rng, (n, c0, h, w))
    bn0 = bn1 = x1 = None
    if xform:
        s0 = rng.choice([-1.0, -0.5, 0.5, 1.0, 2.0], c0).astype(np.float32)
        b0 = (rng.integers(-2, 3, c0) * 0.5).astype(np.float32)
        bn0 = (s0, b0)
        parts.append(np.maximum(x0 * s0[None, :, None, None] + b0[None, :, None, None], 0))
    else:
        parts.append(x0)
    if c1:
        x1 = ints(rng, (n, c1, h, w))
        s1 = rng.choice([-1.0, 0.5, 1.0, 2.0], c1).astype(np.float32)
        b1 = (rng.integers(-2, 3, c1) * 0.5).astype(np.float32)
        bn1 = (s1, b1)
        parts.append(np.maximum(x1 * s1[None, :, None, None] + b1[None, :, None, None], 0))
    eff = np.concatenate(parts, axis=1)
    assert np.array_equal(to_bf16(eff), eff)
    return x0, bn0, x1, bn1, eff.astype(np.float64)


def upload_src(E, c0, c1, x0, bn0, x1, bn1):
    """the engine's source descriptor of what exact_src_host made"""
    st = lambda v: None if v is None else E.BNState(fdev(v[0]), fdev(v[1]))   # noqa: E731
    return E.Src(dev(x0), c0, st(bn0), None if x1 is None else dev(x1), c1, st(bn1))


def exact_src(E, rng, n, h, w, c0, c1, xform):
    x0, bn0, x1, bn1, eff = exact_src_host(rng, n, h, w, c0, c1, xform)
    return upload_src(E, c0, c1, x0, bn0, x1, bn1), eff


def same(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    bad = got != ref
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                           f"{np.unravel_index(bad.argmax(), bad.shape)}: got {got[bad][0]!r} want {ref[bad][0]!r}")
