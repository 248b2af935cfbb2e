"""Data-free helpers of the GPU kernel tests that compare a kernel with a float64 restatement (TEST INFRASTRUCTURE ONLY):
the storage-type rounding, ulps, the three comparison rules and the NaN-tailed output buffer.  Shared by
tests/test_gpu_streaming.py and tests/test_gpu_bn.py so that both hold their kernels to the same rules.

* same          selection / copy kernels and exact operands: bit for bit (NaN matches NaN).
* one_rounding  the float64 result rounded once to the storage type.  bf16: >= 99.9 % equal (one element may differ in a
                tensor of fewer than 1000), every element within 1 bf16 ulp (+ 4 * 2^-24 * sum|terms| where fp32 cancels);
                f32: within max(4 ulp, 4 * 2^-24 * sum|terms|).
* reduced       |got - ref| <= n * 2^-24 * sum|terms| per output (+ 1 ulp of a rounded store).
"""
import zlib

import numpy as np
import torch

PAD = 263                       # tail elements past every output
U = 2.0 ** -24


def seed(*a):
    """a seed that does not depend on the interpreter's string hashing"""
    return zlib.crc32(repr(a).encode())


def stored(a, dt):
    """float64 values as the storage type holds them (one rounding from fp32; fp32 from float64 is one rounding too)"""
    t = torch.from_numpy(np.asarray(a, np.float64).astype(np.float32))
    return t.double().numpy() if dt == "f32" else t.to(torch.bfloat16).double().numpy()


# device inputs live until the test ends: a tensor made inline for a data_ptr() would otherwise go back to the caching
# allocator before the kernel that reads it has run, and the next upload could land in its memory.  The test module
# clears the list in an autouse fixture.
_LIVE = []


class Out:
    """an output tensor inside a longer NaN-filled (or sentinel-filled) buffer"""

    def __init__(self, shape, dtype, fill=float("nan")):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + PAD,), fill, dtype=dtype, device="cuda")
        self.fill = fill
        self.t = self.buf[:self.numel].view(*shape)

    def ptr(self):
        return self.buf.data_ptr()

    def host(self):
        torch.cuda.synchronize()
        tail = self.buf[self.numel:]
        ok = torch.isnan(tail).all() if isinstance(self.fill, float) and np.isnan(self.fill) else (tail == self.fill).all()
        assert bool(ok), "the kernel wrote past the end of its output"
        return self.t.double().cpu().numpy() if self.t.is_floating_point() else self.t.cpu().numpy()


def ulp(v, dt):
    sp = np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)
    return sp * 65536.0 if dt == "bf16" else sp


def same(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.unravel_index(bad.argmax(), bad.shape)}: "
                           f"got {got[bad][0]!r} want {ref[bad][0]!r}")


def one_rounding(got, ref64, terms, dt, what):
    r = stored(ref64, dt)
    got = np.asarray(got, np.float64)
    assert got.shape == r.shape and np.isfinite(got).all(), what
    err = np.abs(got - r)
    cancel = 4 * U * np.asarray(terms, np.float64)
    if dt == "bf16":
        tol = ulp(r, dt) + cancel
        # (a fp32 evaluation can cross a bf16 rounding boundary: one such element is allowed in a small tensor)
        differ = int((got != r).sum())
        assert differ <= max(1, 0.001 * got.size), f"{what}: {differ} of {got.size} elements differ from the once-rounded reference"
    else:
        tol = np.maximum(4 * ulp(r, dt), cancel)
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outside the bound, first at {np.unravel_index(bad.argmax(), bad.shape)}: "
                           f"got {got[bad][0]!r} want {r[bad][0]!r} (tol {tol[bad][0]:.3e})")


def reduced(got, ref64, terms, count, dt, what, stored_dt=None):
    """|got - ref| <= n 2^-24 sum|terms| (n = terms per output) + 1 ulp of the storage rounding"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape and np.isfinite(got).all(), what
    tol = np.asarray(count, np.float64) * U * np.asarray(terms, np.float64) + (ulp(ref64, stored_dt) if stored_dt else 0.0)
    err = np.abs(got - ref64)
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outside the bound, first at {np.unravel_index(bad.argmax(), bad.shape)}: "
                           f"got {got[bad][0]!r} want {ref64[bad][0]!r} (tol {np.broadcast_to(tol, err.shape)[bad][0]:.3e})")
