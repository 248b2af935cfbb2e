"""The BatchNorm / ReLU / 2x2 max-pool backward kernels and the optimizer step of csrc/bn.hip (and oct_reduce_bias_partials)
through the C ABI, on every dispatch path, against the float64 restatements of oracle/ref_bn.py (themselves pinned to torch
by tests/test_oracle_bn.py).  The rules are those of tests/test_gpu_streaming.py (oracle/bounds.py):

* exact operands (small integers, dyadic coefficients): every product and every per-workgroup sum is exact in fp32 in any
  order -- the premise is asserted -- so g, dy, the activations and the float64 sum of the partial rows equal the reference
  bit for bit, also on the LDS-atomic kernels;
* random operands: `one_rounding` for g, dy and the activations, `reduced` for the partial sums with the term count and
  sum |terms| taken from the data (s2 carries three more roundings per term: y - mean, * invstd, * g);
* finalize kernels: 1 fp32 ulp of the reference evaluated on the same fp32 inputs, plus the conditioning of the one subtraction
  each output contains;
* kernels that promise a fixed summation order give the same bits on five calls (not claimed for LDS atomics or dalpha).
Every output lands in a NaN-tailed `Out` buffer; partial rows are NaN-filled before the call.  The row count of every
reduction case is asserted against the kernel the case is meant to reach, so a changed dispatch is noticed.
"""
import numpy as np
import pytest
import torch

from oracle import ref_bn as B
from oracle.bounds import _LIVE, Out, one_rounding, reduced, same, seed, stored, ulp

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
E_INVALID = -22
TINY, TINY_P, MIN_P = (2, 7, 11), (2, 6, 10), (2, 2, 2)
# 2,645,546 pixels of one 16-byte group each (c = 8): more than U * cap * 256 = 4 * 512 * 256 groups, so the unrolled loop, the
# tail loop and the grid cap all run, and the last pass is 42 past a multiple of 256
BIG = (2, 1031, 1283)
# coalesced pooled kernel: 2 * 515 * 1282 = 1,320,460 items > 2048 * 256, 12 past a multiple of 256
BIG_P = (2, 1030, 1282)
# the same with four channel groups per pixel (c = 32): 2,646,644 groups (116 past), 1,319,952 coalesced items (16 past)
BIG32, BIG_P32 = (1, 661, 1001, 32), (2, 514, 642, 32)


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(autouse=True)
def _keep_inputs_alive():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def tdt(dt):
    return torch.float32 if dt == "f32" else torch.bfloat16


def dcode(L, dt):
    return L.DT_F32 if dt == "f32" else L.DT_BF16


def st():
    return torch.cuda.current_stream().cuda_stream


def todev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to("cuda", tdt(dt))
    _LIVE.append(t)
    return t


def f32dev(a):
    return todev(a, "f32")


def P(t):
    return None if t is None else t.data_ptr()


def sid(s):
    return "x".join(map(str, s))


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def refused(L, rc, outs=()):
    assert rc == E_INVALID, rc
    assert L.last_error(), "a refusal carries a message"
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o.buf).all()), "a refused call launched something"


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def coeffs(rng, c, kind, quarter=False):
    """scale, shift, mean, invstd, coef[3][c] as fp32.  exact: scale in {+-0.5, +-1, 2}, shift in halves (+ 0.25: no tie at the
    mask), mean in quarters, invstd a power of two, coefficients in eighths"""
    if kind == "exact":
        sc = rng.choice([0.5, -0.5, 1.0, -1.0, 2.0], c)
        sh = rng.integers(-2, 3, c) * 0.5
        if c >= 2:
            sc[0], sh[0] = 1.0, 0.0           # z == 0 wherever y == 0
        sh = sh + (0.25 if quarter else 0.0)
        mu, inv = rng.integers(-4, 5, c) * 0.25, rng.choice([0.5, 1.0, 2.0], c)
        coef = rng.integers(-8, 9, (3, c)) * 0.125
    else:
        sc = rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c)
        sh = rng.standard_normal(c) * 0.5
        sc[0], sh[0] = 1.0, 0.0
        mu, inv = rng.standard_normal(c) * 0.3, rng.uniform(0.5, 2.0, c)
        coef = rng.standard_normal((3, c))
    return [np.asarray(v, np.float32) for v in (sc, sh, mu, inv, coef)]


def acts(rng, shape, kind, dt):
    if kind == "exact":
        return rng.integers(-3, 4, shape).astype(np.float64)
    y = stored(rng.standard_normal(shape, dtype=np.float32) * 1.5, dt)
    y[..., 0].flat[::5] = 0.0                 # z == 0 exactly in channel 0
    return y


def grads(rng, shape, kind, dt):
    if kind == "exact":
        return rng.integers(-2, 3, shape).astype(np.float64)
    return stored(rng.standard_normal(shape, dtype=np.float32), dt)


def vw(c):
    return 8 if c % 8 == 0 else 1


def expected_rows(kernel, n, h, w, c):
    """the partial rows (= workgroups) of the kernel a case is meant to reach: ceil(work / 256) under the kernel's grid cap"""
    if kernel == "coalesced":                                  # item = (row pair, full-resolution column, 8-channel group)
        work, cap = n * (h // 2) * w * (c // 8), 2048
    elif kernel.startswith("pool"):                            # item = (2x2 window, channel group)
        work, cap = n * (h // 2) * (w // 2) * (c // vw(c)), 512
    else:                                                      # item = (pixel, channel group)
        work, cap = n * h * w * (c // vw(c)), 512
    return min(cap, -(-work // 256)), work


def exact_premise(nblk, work, per_item, *term_arrays, q=8):
    """every partial sum a workgroup can form is an integer multiple of 1/q below 2^24 / q: exact in fp32 in any order.
    A workgroup's channel sees at most passes * 256 thread-iterations of per_item pixels each."""
    passes = -(-work // (nblk * 256))
    for t in term_arrays:
        assert np.array_equal(t * q, np.round(t * q)), f"terms are not multiples of 1/{q}"
        assert passes * 256 * per_item * np.abs(t).max() * q < 2 ** 24


# ------------------------------------------------------------------------------------------------------------------
# oct_dact_bn_reduce: every kernel it can choose
# ------------------------------------------------------------------------------------------------------------------
FIXED = {"coalesced", "flat", "pool-reg", "gen-reg"}      # register sums, combined in a fixed order
RED = [(TINY_P + (c,), "coalesced") for c in (8, 32, 256)] + [(MIN_P + (c,), "coalesced") for c in (8, 32, 256)] + \
      [(TINY_P + (512,), "pool-reg"), (TINY_P + (24,), "pool-lds"), (TINY_P + (96,), "pool-lds"), (TINY_P + (4,), "pool-reg"),
       (TINY_P + (3,), "pool-lds"), (MIN_P + (512,), "pool-reg"), (MIN_P + (24,), "pool-lds"), (MIN_P + (96,), "pool-lds"),
       (MIN_P + (4,), "pool-reg"), (MIN_P + (3,), "pool-lds"),
       ((1, 100, 100, 512), "pool-reg"), ((2, 302, 422, 4), "pool-reg"), ((2, 302, 422, 3), "pool-lds"),     # grid cap 512
       (BIG_P + (8,), "coalesced"), (BIG_P32, "coalesced")] + \
      [(TINY + (c,), "flat") for c in (8, 64, 512)] + [(TINY + (24,), "gen-lds"), (TINY + (1,), "gen-reg"), (TINY + (3,), "gen-lds"),
                                                      ((2, 151, 211, 3), "gen-lds"), (BIG + (8,), "flat"), (BIG32, "flat")]
ROWS = {(TINY_P + (8,), "coalesced"): 1, (TINY_P + (256,), "coalesced"): 8, (TINY_P + (512,), "pool-reg"): 8,
        (TINY_P + (96,), "pool-lds"): 2, ((1, 100, 100, 512), "pool-reg"): 512, ((2, 302, 422, 3), "pool-lds"): 512,
        (BIG_P + (8,), "coalesced"): 2048, (BIG_P32, "coalesced"): 2048, (BIG32, "flat"): 512, (TINY + (64,), "flat"): 5, (TINY + (512,), "flat"): 39, (TINY + (24,), "gen-lds"): 2,
        ((2, 151, 211, 3), "gen-lds"): 512, (BIG + (8,), "flat"): 512}       # a few of them spelled out
RED_CASES = [(s, k, kind, q) for s, k in RED for kind, q in (("exact", False), ("exact", True), ("random", False))
             if not (np.prod(s) > 2 ** 22 and q)]


def _rows(part, nblk, c):
    r = part.host()
    assert r.shape == (nblk, 2, c) and np.isfinite(r).all(), "a partial row was not written"
    return r


def _check_rows(rows, ref, kind, dt, what):
    tot = rows.sum(0)
    if kind == "exact":
        same(tot[0], ref["s1"], what + ": sum g (exact operands)")
        same(tot[1], ref["s2"], what + ": sum g*xhat (exact operands)")
    else:
        reduced(tot[0], ref["s1"], ref["t1"], ref["count"], dt, what + ": sum g")
        reduced(tot[1], ref["s2"], ref["t2"], ref["count"] + 3, dt, what + ": sum g*xhat")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,kernel,kind,quarter", RED_CASES, ids=[f"{sid(s)}-{k}-{kind}{'-q' if q else ''}" for s, k, kind, q in RED_CASES])
def test_dact_bn_reduce(L, dt, shape, kernel, kind, quarter):
    lib = L.lib()
    n, h, w, c = shape
    pooled = kernel == "coalesced" or kernel.startswith("pool")
    big = np.prod(shape) > 2 ** 22
    nblk = lib.oct_dact_bn_reduce_blocks(n, h, w, c, int(pooled))
    want, work = expected_rows(kernel, n, h, w, c)
    assert nblk == want == ROWS.get((shape, kernel), want), f"{kernel}: {nblk} partial rows, expected {want}"
    assert lib.oct_bn_bwd_apply_pool_ok(dcode(L, dt), n, h, w, c) == int(kernel == "coalesced") or not pooled
    per_item = 2 if kernel == "coalesced" else 4 if pooled else 1
    store = lambda v: stored(v, dt)                                          # noqa: E731
    for use_da in ((True, False) if pooled and not big else (True,)):
        rng = np.random.default_rng(seed(shape, kernel, kind, quarter, use_da, dt))
        sc, sh, mu, inv, _ = coeffs(rng, c, kind, quarter)
        y = acts(rng, shape, kind, dt)
        da = grads(rng, shape, kind, dt) if use_da else None
        dp = grads(rng, (n, h // 2, w // 2, c), kind, dt) if pooled else None
        ref = B.dact_bn_reduce(da, dp, y, sc, sh, mu, inv, store)
        if kind == "exact":
            xhat = (y - mu.astype(np.float64)) * inv.astype(np.float64)
            exact_premise(nblk, work, per_item, ref["g"], ref["g"] * xhat)
            if not quarter and c >= 2:
                assert (B.z32(y, sc, sh) == 0).any(), "no tie at the mask"
        yd, dad, dpd = todev(y, dt), (todev(da, dt) if use_da else None), (todev(dp, dt) if pooled else None)
        keep = [t.clone() if t is not None else None for t in (yd, dad, dpd)]
        vec = [f32dev(v) for v in (sc, sh, mu, inv)]
        tag = f"{kernel} da={use_da} dpool={pooled}"

        def call(g_ptr, da_ptr):
            part = Out((nblk, 2, c), torch.float32)
            L.check(lib.oct_dact_bn_reduce(dcode(L, dt), da_ptr, P(dpd), P(yd), *[P(v) for v in vec], g_ptr, part.ptr(), n, h, w, c, st()),
                    "oct_dact_bn_reduce")
            return part

        g0 = Out(shape, tdt(dt))
        rows0 = _rows(call(g0.ptr(), P(dad)), nblk, c)
        got = g0.host()
        if kind == "exact":
            same(got, ref["g"], tag + ": g (routing and masking are selections)")
        else:
            one_rounding(got, ref["g"], np.abs(ref["g"]), dt, tag + ": g")
        _check_rows(rows0, ref, kind, dt, tag)
        if kernel in FIXED:
            for _ in range(4):
                g = Out(shape, tdt(dt))
                same(_rows(call(g.ptr(), P(dad)), nblk, c), rows0, tag + ": partial rows, repeated (fixed order)")
                assert torch.equal(bits(g.t), bits(g0.t)), tag + ": g, repeated"
        # the reduce-only pass writes no g; nothing else changes
        if not pooled or kernel == "coalesced":
            rows = _rows(call(None, P(dad)), nblk, c)
            if kernel in FIXED:
                same(rows, rows0, tag + ": reduce-only partial rows")
            else:
                _check_rows(rows, ref, kind, dt, tag + " reduce-only")
        for t, k in zip((yd, dad, dpd), keep):
            assert t is None or torch.equal(bits(t), bits(k)), "an input was modified"
        if use_da:                                                            # g may alias da
            ga = Out(shape, tdt(dt))
            ga.t.copy_(dad)
            rows = _rows(call(ga.ptr(), ga.ptr()), nblk, c)
            assert torch.equal(bits(ga.t), bits(g0.t)), tag + ": g aliasing da"
            ga.host()
            if kernel in FIXED:
                same(rows, rows0, tag + ": partial rows with g aliasing da")
            else:
                _check_rows(rows, ref, kind, dt, tag + " aliased")


def test_dact_bn_reduce_refusals(L):
    lib = L.lib()
    n, h, w, c = 2, 6, 10, 24
    t = torch.zeros((n, h, w, c), device="cuda")
    v = torch.ones(c, device="cuda")
    g, part = Out((n, h, w, c), torch.float32), Out((512, 2, c), torch.float32)
    a = [v.data_ptr()] * 4

    def red(da, dp, y, g_ptr, hh=h, ww=w, cc=c, sc=a):
        return lib.oct_dact_bn_reduce(L.DT_F32, da, dp, y, *sc, g_ptr, part.ptr(), n, hh, ww, cc, st())

    refused(L, red(t.data_ptr(), t.data_ptr(), t.data_ptr(), g.ptr(), hh=5), (g, part))            # odd h with dpool
    refused(L, red(t.data_ptr(), t.data_ptr(), t.data_ptr(), g.ptr(), ww=9), (g, part))            # odd w with dpool
    assert lib.oct_bn_bwd_apply_pool_ok(L.DT_F32, n, h, w, c) == 0
    refused(L, red(t.data_ptr(), t.data_ptr(), t.data_ptr(), None), (g, part))                     # pooled reduce-only, not eligible
    refused(L, red(None, None, t.data_ptr(), g.ptr()), (g, part))                                  # neither da nor dpool
    refused(L, red(t.data_ptr(), None, None, g.ptr()), (g, part))                                  # y
    refused(L, red(t.data_ptr(), None, t.data_ptr(), g.ptr(), sc=[None] + a[1:]), (g, part))       # scale
    refused(L, lib.oct_dact_bn_reduce(L.DT_F32, t.data_ptr(), None, t.data_ptr(), *a, g.ptr(), None, n, h, w, c, st()), (g,))
    refused(L, lib.oct_dact_bn_reduce(7, t.data_ptr(), None, t.data_ptr(), *a, g.ptr(), part.ptr(), n, h, w, c, st()), (g, part))
    coef = torch.zeros((3, c), device="cuda")
    refused(L, lib.oct_bn_bwd_apply_pool(L.DT_F32, t.data_ptr(), t.data_ptr(), t.data_ptr(), a[0], a[1], coef.data_ptr(), g.ptr(), n, h, w, c, st()), (g,))
    refused(L, lib.oct_bn_bwd_apply_pool(L.DT_F32, t.data_ptr(), None, t.data_ptr(), a[0], a[1], coef.data_ptr(), g.ptr(), n, h, w, 8, st()), (g,))
    # apply: scale without shift, null pointers
    refused(L, lib.oct_bn_bwd_apply_to(L.DT_F32, g.ptr(), t.data_ptr(), t.data_ptr(), coef.data_ptr(), a[0], None, n * h * w, c, st()), (g,))
    refused(L, lib.oct_bn_bwd_apply_to(L.DT_F32, g.ptr(), t.data_ptr(), t.data_ptr(), coef.data_ptr(), None, a[0], n * h * w, c, st()), (g,))
    refused(L, lib.oct_bn_bwd_apply_to(L.DT_F32, g.ptr(), None, t.data_ptr(), coef.data_ptr(), None, None, n * h * w, c, st()), (g,))
    refused(L, lib.oct_bn_bwd_apply_to(L.DT_F32, g.ptr(), t.data_ptr(), t.data_ptr(), None, None, None, n * h * w, c, st()), (g,))
    refused(L, lib.oct_bn_bwd_apply(L.DT_F32, None, t.data_ptr(), coef.data_ptr(), None, None, n * h * w, c, st()))
    # forward
    refused(L, lib.oct_bn_relu_fwd(L.DT_F32, t.data_ptr(), a[0], None, g.ptr(), n * h * w, c, st()), (g,))
    refused(L, lib.oct_bn_relu_pool_fwd(L.DT_F32, t.data_ptr(), a[0], a[1], g.ptr(), n, 5, w, c, st()), (g,))
    refused(L, lib.oct_bn_relu_pool_fwd(L.DT_F32, None, a[0], a[1], g.ptr(), n, h, w, c, st()), (g,))
    # the optimizer: momentum without a buffer, null pointers
    refused(L, lib.oct_sgd_step(g.ptr(), t.data_ptr(), None, 16, 0.1, 0.9, 0.0, 1.0, 0, st()), (g,))
    refused(L, lib.oct_sgd_step(None, t.data_ptr(), None, 16, 0.1, 0.0, 0.0, 1.0, 0, st()))
    refused(L, lib.oct_sgd_step(g.ptr(), None, None, 16, 0.1, 0.0, 0.0, 1.0, 0, st()), (g,))
    # finalize kernels
    o = [Out((c,), torch.float32) for _ in range(4)]
    refused(L, lib.oct_bn_finalize(None, 1, c, 4.0, a[0], a[0], 1e-5, 0.1, None, None, *[x.ptr() for x in o], None, st()), o)
    refused(L, lib.oct_bn_finalize(part.ptr(), 1, c, 4.0, a[0], a[0], 1e-5, 0.1, o[0].ptr(), None, *[x.ptr() for x in o], None, st()), o)
    refused(L, lib.oct_bn_bwd_finalize(part.ptr(), 1, c, 4.0, a[0], a[0], None, o[0].ptr(), o[1].ptr(), g.ptr(), 0, st()), o[:2] + [g])
    refused(L, lib.oct_bn_eval_coeffs(c, a[0], a[0], a[0], None, 1e-5, o[0].ptr(), o[1].ptr(), None, st()), o[:2])
    refused(L, lib.oct_reduce_bias_partials(part.ptr(), 2, 7, 3, o[0].ptr(), 0, st()), o[:1])          # rows not a multiple of channels
    refused(L, lib.oct_reduce_bias_partials(None, 2, 6, 3, o[0].ptr(), 0, st()), o[:1])


# ------------------------------------------------------------------------------------------------------------------
# oct_bn_bwd_apply / _to (flat against general kernel) and oct_bn_bwd_apply_pool
# ------------------------------------------------------------------------------------------------------------------
APPLY = [(TINY + (c,), k) for c, k in ((8, "flat"), (64, "flat"), (512, "flat"), (24, "general"), (1, "general"), (3, "general"))] + \
        [((2, 151, 211, 3), "general"), (BIG + (8,), "flat"), (BIG32, "flat")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape,kernel", APPLY, ids=[f"{sid(s)}-{k}" for s, k in APPLY])
def test_bn_bwd_apply(L, dt, shape, kernel, masked, kind):
    lib = L.lib()
    n, h, w, c = shape
    npix = n * h * w
    assert (kernel == "flat") == (c % 8 == 0 and 256 % (c // 8) == 0)
    rng = np.random.default_rng(seed(shape, masked, kind, dt))
    sc, sh, _, _, coef = coeffs(rng, c, kind)
    y, g = acts(rng, shape, kind, dt), grads(rng, shape, kind, dt)
    ref, terms = B.bn_bwd_apply(g, y, coef, sc if masked else None, sh if masked else None)
    yd, gd, cd = todev(y, dt), todev(g, dt), f32dev(coef)
    scd, shd = (f32dev(sc), f32dev(sh)) if masked else (None, None)
    gkeep = gd.clone()
    first = None
    for _ in range(5):                                           # element-wise: the same bits every call
        dy = Out(shape, tdt(dt))
        L.check(lib.oct_bn_bwd_apply_to(dcode(L, dt), dy.ptr(), P(gd), P(yd), P(cd), P(scd), P(shd), npix, c, st()))
        if first is None:
            first = dy
            got = dy.host()
            if kind == "exact":
                same(got, stored(ref, dt), "bn_bwd_apply_to (exact operands)")
            else:
                one_rounding(got, ref, terms, dt, "bn_bwd_apply_to")
        else:
            dy.host()
            assert torch.equal(bits(dy.t), bits(first.t)), "bn_bwd_apply_to, repeated"
    assert torch.equal(bits(gd), bits(gkeep)), "dst != g: g must come back unchanged"
    for entry in ("to", "inplace"):                              # dst == g through both entry points
        io = Out(shape, tdt(dt))
        io.t.copy_(gd)
        if entry == "to":
            L.check(lib.oct_bn_bwd_apply_to(dcode(L, dt), io.ptr(), io.ptr(), P(yd), P(cd), P(scd), P(shd), npix, c, st()))
        else:
            L.check(lib.oct_bn_bwd_apply(dcode(L, dt), io.ptr(), P(yd), P(cd), P(scd), P(shd), npix, c, st()))
        io.host()
        assert torch.equal(bits(io.t), bits(first.t)), f"bn_bwd_apply ({entry}), dst == g"


KINDS = [("exact", False), ("exact", True), ("random", False)]


def with_kinds(shapes):
    """every shape with the three kinds of data; the large ones once per kind"""
    cases = [(s, kind, q) for s in shapes for kind, q in KINDS if not (np.prod(s) > 2 ** 22 and q)]
    return dict(argnames="shape,kind,quarter", argvalues=cases, ids=[f"{sid(s)}-{kind}{'-q' if q else ''}" for s, kind, q in cases])


POOL_APPLY = [(TINY_P + (c,)) for c in (8, 32, 256)] + [(MIN_P + (c,)) for c in (8, 32, 256)] + [BIG_P + (8,), BIG_P32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize(**with_kinds(POOL_APPLY))
def test_bn_bwd_apply_pool(L, dt, shape, kind, quarter):
    lib = L.lib()
    n, h, w, c = shape
    big = np.prod(shape) > 2 ** 22
    assert lib.oct_bn_bwd_apply_pool_ok(dcode(L, dt), n, h, w, c) == 1
    for use_da in ((True,) if big else (True, False)):
        rng = np.random.default_rng(seed(shape, kind, quarter, use_da, dt))
        sc, sh, _, _, coef = coeffs(rng, c, kind, quarter)
        y = acts(rng, shape, kind, dt)
        da = grads(rng, shape, kind, dt) if use_da else None
        dp = grads(rng, (n, h // 2, w // 2, c), kind, dt)
        ref, terms = B.bn_bwd_apply_pool(da, dp, y, sc, sh, coef, lambda v: stored(v, dt))
        yd, dpd, dad = todev(y, dt), todev(dp, dt), (todev(da, dt) if use_da else None)
        scd, shd, cd = f32dev(sc), f32dev(sh), f32dev(coef)
        first = None
        for _ in range(5):
            dy = Out(shape, tdt(dt))
            L.check(lib.oct_bn_bwd_apply_pool(dcode(L, dt), P(dad), P(dpd), P(yd), P(scd), P(shd), P(cd), dy.ptr(), n, h, w, c, st()))
            if first is None:
                first = dy
                if kind == "exact":
                    same(dy.host(), stored(ref, dt), "bn_bwd_apply_pool (exact operands)")
                else:
                    one_rounding(dy.host(), ref, terms, dt, "bn_bwd_apply_pool")
            else:
                dy.host()
                assert torch.equal(bits(dy.t), bits(first.t)), "bn_bwd_apply_pool, repeated"
        if use_da:                                               # dy may alias da
            io = Out(shape, tdt(dt))
            io.t.copy_(dad)
            L.check(lib.oct_bn_bwd_apply_pool(dcode(L, dt), io.ptr(), P(dpd), P(yd), P(scd), P(shd), P(cd), io.ptr(), n, h, w, c, st()))
            io.host()
            assert torch.equal(bits(io.t), bits(first.t)), "bn_bwd_apply_pool, dy aliasing da"


# ------------------------------------------------------------------------------------------------------------------
# forward: relu(bn(y)) materialised, and its 2x2 max-pool
# ------------------------------------------------------------------------------------------------------------------
FWD = [TINY + (c,) for c in (8, 64, 512, 24, 1, 3)] + [BIG + (8,), (2, 151, 211, 3)]
FWD_P = [TINY_P + (c,) for c in (8, 32, 256, 512, 24, 96, 4, 3)] + [MIN_P + (c,) for c in (8, 512, 24, 4, 3)] + \
        [BIG_P + (8,), (2, 302, 422, 3)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize(**with_kinds(FWD))
def test_bn_relu_fwd(L, dt, shape, kind, quarter):
    n, h, w, c = shape
    rng = np.random.default_rng(seed(shape, kind, quarter, dt))
    sc, sh, _, _, _ = coeffs(rng, c, kind, quarter)
    y = acts(rng, shape, kind, dt)
    ref, terms, z = B.bn_relu(y, sc, sh)
    assert quarter or c < 2 or (z == 0).any()
    out = Out(shape, tdt(dt))
    L.check(L.lib().oct_bn_relu_fwd(dcode(L, dt), P(todev(y, dt)), P(f32dev(sc)), P(f32dev(sh)), out.ptr(), n * h * w, c, st()))
    if kind == "exact":
        same(out.host(), stored(ref, dt), "bn_relu_fwd (exact operands)")
    else:
        one_rounding(out.host(), ref, terms, dt, "bn_relu_fwd")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize(**with_kinds(FWD_P))
def test_bn_relu_pool_fwd(L, dt, shape, kind, quarter):
    n, h, w, c = shape
    rng = np.random.default_rng(seed(shape, kind, quarter, dt))
    sc, sh, _, _, _ = coeffs(rng, c, kind, quarter)
    y = acts(rng, shape, kind, dt)
    ref, terms, _ = B.bn_relu_pool(y, sc, sh)
    out = Out(ref.shape, tdt(dt))
    L.check(L.lib().oct_bn_relu_pool_fwd(dcode(L, dt), P(todev(y, dt)), P(f32dev(sc)), P(f32dev(sh)), out.ptr(), n, h, w, c, st()))
    if kind == "exact":
        same(out.host(), stored(ref, dt), "bn_relu_pool_fwd (exact operands)")
    else:
        one_rounding(out.host(), ref, terms, dt, "bn_relu_pool_fwd")


def nan_input(rng, shape, dt):
    """NaN in the first, a middle and the last slot of 2x2 windows, in the first and the last channel of a vector group"""
    n, h, w, c = shape
    y = stored(rng.standard_normal(shape) * 1.5, dt)
    y[0, 0, 0, 0] = np.nan                       # first slot, first channel
    y[0, 0, 3, c - 1] = np.nan                   # second slot, last channel
    y[0, 3, 4, min(7, c - 1)] = np.nan           # third slot, last channel of the first group
    y[-1, h - 1, w - 1, c - 1] = np.nan          # last slot of the last window
    y[-1, 2, 2, (c // 2 // 8) * 8] = np.nan      # first channel of a middle group
    return y


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [8, 64, 24, 3, 1])
def test_nan_survives_the_materialised_activation(L, dt, c):
    """torch: relu(NaN) is NaN and a window that holds one pools to NaN -- also through a NaN scale.  Elsewhere nothing changes."""
    lib = L.lib()
    shape = TINY_P + (c,)
    n, h, w, _ = shape
    rng = np.random.default_rng(seed("nan", c, dt))
    sc, sh, _, _, _ = coeffs(rng, c, "random")
    y = nan_input(rng, shape, dt)
    clean = np.where(np.isnan(y), 0.0, y)
    for nan_scale in ((False, True) if c > 1 else (False,)):
        s = sc.copy()
        if nan_scale:
            s[c // 2] = np.nan
        t = torch.from_numpy(y * s.astype(np.float64) + sh.astype(np.float64)).permute(0, 3, 1, 2)
        ta = torch.relu(t)
        want_a = ta.permute(0, 2, 3, 1).numpy()
        want_p = torch.nn.functional.max_pool2d(ta, 2).permute(0, 2, 3, 1).numpy()
        assert np.isnan(want_a).sum() >= (5 if c > 1 else 3) and np.isnan(want_p).any() and not np.isnan(want_p).all()
        s_clean = np.where(np.isnan(s), 1.0, s)
        yd, sd, shd = todev(y, dt), f32dev(s), f32dev(sh)
        a = Out(shape, tdt(dt))
        L.check(lib.oct_bn_relu_fwd(dcode(L, dt), P(yd), P(sd), P(shd), a.ptr(), n * h * w, c, st()))
        got = a.host()
        assert np.array_equal(np.isnan(got), np.isnan(want_a)), "bn_relu_fwd: NaN where torch.relu has NaN, nowhere else"
        ref, terms, _ = B.bn_relu(clean, s_clean, sh)
        ok = ~np.isnan(want_a)
        one_rounding(np.where(ok, got, 0.0), np.where(ok, ref, 0.0), terms, dt, "bn_relu_fwd away from the NaNs")
        p = Out(want_p.shape, tdt(dt))
        L.check(lib.oct_bn_relu_pool_fwd(dcode(L, dt), P(yd), P(sd), P(shd), p.ptr(), n, h, w, c, st()))
        got = p.host()
        assert np.array_equal(np.isnan(got), np.isnan(want_p)), "bn_relu_pool_fwd: NaN where max_pool2d(relu(.)) has NaN, nowhere else"
        ref, terms, _ = B.bn_relu_pool(clean, s_clean, sh)
        ok = ~np.isnan(want_p)
        one_rounding(np.where(ok, got, 0.0), np.where(ok, ref, 0.0), terms, dt, "bn_relu_pool_fwd away from the NaNs")


# ------------------------------------------------------------------------------------------------------------------
# the PReLU pair
# ------------------------------------------------------------------------------------------------------------------
PRELU = [TINY + (c,) for c in (8, 64, 512)] + [BIG + (8,), BIG32]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize(**with_kinds(PRELU))
def test_prelu_bn_backward_pair(L, dt, shape, kind, quarter):
    lib = L.lib()
    n, h, w, c = shape
    npix = n * h * w
    assert lib.oct_prelu_bn_fused_ok(dcode(L, dt), c) == 1
    rng = np.random.default_rng(seed(shape, kind, quarter, dt))
    sc, sh, mu, inv, coef = coeffs(rng, c, kind, quarter)
    alpha = np.array([0.25], np.float32)
    y, da = acts(rng, shape, kind, dt), grads(rng, shape, kind, dt)
    store = lambda v: stored(v, dt)                                          # noqa: E731
    ref = B.dact_bn_reduce_prelu(da, y, sc, sh, alpha[0], mu, inv, store)
    assert quarter or (ref["z"] == 0).any()
    nblk = lib.oct_dact_bn_reduce_blocks(n, h, w, c, 0)
    want, work = expected_rows("flat", n, h, w, c)
    assert nblk == want
    yd, dad = todev(y, dt), todev(da, dt)
    vec = [f32dev(v) for v in (sc, sh, alpha, mu, inv)]
    rows0 = None
    for _ in range(5):
        part, dal = Out((nblk, 2, c), torch.float32), Out((1,), torch.float32)
        dal.t.zero_()
        L.check(lib.oct_dact_bn_reduce_prelu(dcode(L, dt), P(dad), P(yd), *[P(v) for v in vec], part.ptr(), dal.ptr(), n, h, w, c, st()))
        rows = _rows(part, nblk, c)
        if rows0 is None:
            rows0 = rows
            if kind == "exact":
                xhat = (y - mu.astype(np.float64)) * inv.astype(np.float64)
                exact_premise(nblk, work, 1, ref["g"], ref["g"] * xhat, q=32)      # dz in quarters (alpha = 0.25), xhat in eighths
            _check_rows(rows, ref, kind, dt, "dact_bn_reduce_prelu")
        else:
            same(rows, rows0, "dact_bn_reduce_prelu partial rows, repeated (fixed order)")
        # dalpha: one global fp32 atomic per wave, no order promised -- exact only while every partial sum is
        if kind == "exact" and ref["dalpha_terms"] * 4 < 2 ** 24:
            same(dal.host(), np.array([ref["dalpha"]]), "dalpha (exact operands)")
        else:
            reduced(dal.host(), np.array([ref["dalpha"]]), np.array([ref["dalpha_terms"]]), npix * c + 1, dt, "dalpha")
    rdy, terms = B.bn_bwd_apply_prelu(da, y, coef, sc, sh, alpha[0], store)
    cd, dkeep = f32dev(coef), dad.clone()
    first = None
    for _ in range(5):
        dy = Out(shape, tdt(dt))
        L.check(lib.oct_bn_bwd_apply_prelu_to(dcode(L, dt), dy.ptr(), P(dad), P(yd), P(cd), P(vec[0]), P(vec[1]), P(vec[2]), npix, c, st()))
        if first is None:
            first = dy
            if kind == "exact":
                same(dy.host(), stored(rdy, dt), "bn_bwd_apply_prelu_to (exact operands)")
            else:
                one_rounding(dy.host(), rdy, terms, dt, "bn_bwd_apply_prelu_to")
        else:
            dy.host()
            assert torch.equal(bits(dy.t), bits(first.t)), "bn_bwd_apply_prelu_to, repeated"
    assert torch.equal(bits(dad), bits(dkeep)), "da must come back unchanged"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [24, 3, 520])
def test_prelu_pair_refuses_other_channel_counts(L, dt, c):
    lib = L.lib()
    assert lib.oct_prelu_bn_fused_ok(dcode(L, dt), c) == 0
    n, h, w = TINY
    t = torch.zeros((n, h, w, c), dtype=tdt(dt), device="cuda")
    v = torch.ones(3 * c, device="cuda")
    part, dal, dy = Out((512, 2, c), torch.float32), Out((1,), torch.float32), Out((n, h, w, c), tdt(dt))
    p = v.data_ptr()
    refused(L, lib.oct_dact_bn_reduce_prelu(dcode(L, dt), P(t), P(t), p, p, p, p, p, part.ptr(), dal.ptr(), n, h, w, c, st()), (part, dal))
    refused(L, lib.oct_bn_bwd_apply_prelu_to(dcode(L, dt), dy.ptr(), P(t), P(t), p, p, p, p, n * h * w, c, st()), (dy,))


# ------------------------------------------------------------------------------------------------------------------
# finalize kernels: the reference on the same fp32 rows and vectors
# ------------------------------------------------------------------------------------------------------------------
E53 = 2.0 ** -53


def within(got, ref, cond, what, ulps=1):
    """|got - ref| <= ulps fp32 ulps of the reference + the conditioning term"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    tol = ulps * ulp(ref, "f32") + np.asarray(cond, np.float64)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{what}: got {got[bad][0]!r} want {ref[bad][0]!r} (tol {np.broadcast_to(tol, got.shape)[bad][0]:.3e})"


def stat_rows(rng, nblocks, c, sigmas, per_block=64):
    """fp32 rows [nblocks][2][c] of a channel whose mean lies `sigmas` standard deviations from zero, built in float64"""
    std = rng.uniform(0.5, 2.0, c)
    m = std * sigmas * rng.choice([-1, 1], c)
    mu_b = m + 0.1 * std * rng.standard_normal((nblocks, c))
    var_b = std ** 2 * rng.uniform(0.8, 1.2, (nblocks, c))
    rows = np.stack([per_block * mu_b, per_block * (var_b + mu_b ** 2)], 1)
    return rows.astype(np.float32), float(nblocks * per_block)


FIN = [(nb, sg, rs, cb) for nb in (1, 255, 256, 257, 2048) for sg in (1, 30, 1000) for rs, cb in ((True, True), (True, False), (False, False))]


@pytest.mark.parametrize("nblocks,sigmas,running,bias", FIN + [(1, 0, True, True)], ids=lambda v: str(v))
def test_bn_finalize(L, nblocks, sigmas, running, bias):
    lib = L.lib()
    c = 37
    rng = np.random.default_rng(seed("fin", nblocks, sigmas, running, bias))
    if sigmas == 0:                                               # count = 1: one value per channel
        v = rng.standard_normal(c)
        rows, count = np.stack([v, v * v])[None].astype(np.float32), 1.0
    else:
        rows, count = stat_rows(rng, nblocks, c, sigmas)
    gamma, beta = (1 + 0.3 * rng.standard_normal(c)).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    cb = rng.standard_normal(c).astype(np.float32) if bias else None
    rm0, rv0 = rng.standard_normal(c).astype(np.float32), rng.uniform(0.5, 2, c).astype(np.float32)
    eps, mom = float(np.float32(1e-5)), float(np.float32(0.1))
    ref = B.bn_finalize(rows, count, gamma, beta, eps, mom, cb, rm0 if running else None, rv0 if running else None)
    outs = [Out((c,), torch.float32) for _ in range(4)]
    rmd, rvd = Out((c,), torch.float32), Out((c,), torch.float32)
    rmd.t.copy_(torch.from_numpy(rm0))
    rvd.t.copy_(torch.from_numpy(rv0))
    L.check(lib.oct_bn_finalize(P(f32dev(rows)), nblocks, c, count, P(f32dev(gamma)), P(f32dev(beta)), eps, mom,
                                rmd.ptr() if running else None, rvd.ptr() if running else None, *[o.ptr() for o in outs],
                                P(f32dev(cb)) if bias else None, st()))
    mean, invstd, scale, shift = [o.host() for o in outs]
    r64 = rows.astype(np.float64)
    # double sums of nblocks terms, then var = s2/count - mean^2: the one subtraction
    dsum = (nblocks + 4) * E53
    dmean = dsum * np.abs(r64[:, 0]).sum(0) / count
    dvar = dsum * (np.abs(r64[:, 1]).sum(0) / count + ref["mean"] ** 2) + 2 * np.abs(ref["mean"]) * dmean
    dinv = 0.5 * ref["invstd"] ** 3 * dvar
    within(mean, ref["mean"], dmean, "mean")
    within(invstd, ref["invstd"], dinv, "invstd")
    within(scale, ref["scale"], np.abs(gamma) * dinv, "scale")
    dshift = np.abs(ref["mean"] * gamma) * dinv + np.abs(ref["scale"]) * dmean + 4 * E53 * (np.abs(beta) + np.abs(ref["mean"] * ref["scale"]))
    within(shift, ref["shift"], dshift, "shift = beta - mean*scale")
    if running:
        within(rmd.host(), ref["running_mean"], mom * dmean, "running_mean")
        k = count / (count - 1.0) if count > 1 else 1.0
        within(rvd.host(), ref["running_var"], mom * k * dvar, "running_var")
        if count == 1.0:
            assert (ref["var"] < 1e-6).all()
    else:
        same(rmd.host(), rm0, "running_mean untouched")
        same(rvd.host(), rv0, "running_var untouched")


BFIN = [(nb, sg, acc) for nb in (1, 255, 256, 257, 2048) for sg in (1, 30, 1000) for acc in (0, 1)]


@pytest.mark.parametrize("nblocks,sigmas,accumulate", BFIN)
def test_bn_bwd_finalize(L, nblocks, sigmas, accumulate):
    lib = L.lib()
    c = 37
    rng = np.random.default_rng(seed("bfin", nblocks, sigmas, accumulate))
    rows = (rng.standard_normal((nblocks, 2, c)) * 8).astype(np.float32)
    count = float(nblocks * 64)
    gamma = (1 + 0.3 * rng.standard_normal(c)).astype(np.float32)
    invstd = rng.uniform(0.5, 2.0, c).astype(np.float32)
    mean = (sigmas / invstd.astype(np.float64) * rng.choice([-1, 1], c)).astype(np.float32)
    dg0, db0 = rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    ref = B.bn_bwd_finalize(rows, count, gamma, mean, invstd, dg0, db0, bool(accumulate))
    dg, db, coef = Out((c,), torch.float32), Out((c,), torch.float32), Out((3, c), torch.float32)
    if accumulate:
        dg.t.copy_(torch.from_numpy(dg0))
        db.t.copy_(torch.from_numpy(db0))
    L.check(lib.oct_bn_bwd_finalize(P(f32dev(rows)), nblocks, c, count, P(f32dev(gamma)), P(f32dev(mean)), P(f32dev(invstd)),
                                    dg.ptr(), db.ptr(), coef.ptr(), accumulate, st()))
    r64 = np.abs(rows.astype(np.float64))
    dsum = (nblocks + 4) * E53
    d1, d2 = dsum * r64[:, 0].sum(0), dsum * r64[:, 1].sum(0)
    # accumulate: dgamma += (float)s2 is two fp32 roundings, the first of them at the magnitude of the sum alone
    extra2 = ulp(ref["s2"], "f32") if accumulate else 0.0
    extra1 = ulp(ref["s1"], "f32") if accumulate else 0.0
    within(dg.host(), ref["dgamma"], d2 + extra2, "dgamma")
    within(db.host(), ref["dbeta"], d1 + extra1, "dbeta")
    got = coef.host()
    a = np.abs(ref["coef"][0])
    within(got[0], ref["coef"][0], 0.0, "k0 = gamma*invstd")
    dk1 = a * invstd * d2 / count + 4 * E53 * np.abs(ref["coef"][1])
    within(got[1], ref["coef"][1], dk1, "k1")
    within(got[2], ref["coef"][2], a * d1 / count + dk1 * np.abs(mean) + 4 * E53 * ref["k2_terms"], "k2 = -a*mg - k1*mean")


@pytest.mark.parametrize("sigmas", [1, 30, 1000])
@pytest.mark.parametrize("bias", [False, True])
def test_bn_eval_coeffs(L, sigmas, bias):
    """fp32 arithmetic: scale = gamma / sqrtf(rv + eps) is three roundings (add, sqrt, divide); shift = beta - (rm - b) * scale
    adds a subtraction and one fma: five, each relative to the larger addend of the subtraction it feeds"""
    c = 300                                                       # two workgroups
    rng = np.random.default_rng(seed("eval", sigmas, bias))
    gamma, beta = (1 + 0.3 * rng.standard_normal(c)).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    rv = rng.uniform(0.3, 3.0, c).astype(np.float32)
    rm = (np.sqrt(rv) * sigmas * rng.choice([-1, 1], c)).astype(np.float32)
    cb = rng.standard_normal(c).astype(np.float32) if bias else None
    eps = float(np.float32(1e-5))
    rs, rsh = B.bn_eval_coeffs(gamma, beta, rm, rv, eps, cb)
    sc, sh = Out((c,), torch.float32), Out((c,), torch.float32)
    L.check(L.lib().oct_bn_eval_coeffs(c, P(f32dev(gamma)), P(f32dev(beta)), P(f32dev(rm)), P(f32dev(rv)), eps, sc.ptr(), sh.ptr(),
                                       P(f32dev(cb)) if bias else None, st()))
    within(sc.host(), rs, 0.0, "scale", ulps=3)
    m = np.abs(rm.astype(np.float64)) + (np.abs(cb.astype(np.float64)) if bias else 0.0)
    within(sh.host(), rsh, 5 * 2.0 ** -23 * (np.abs(beta) + m * np.abs(rs)), "shift", ulps=1)


BIAS = [(1, 8, 8), (7, 24, 24), (5, 24, 6), (33, 1200, 300), (2048, 12, 3), (3, 300, 300)]


@pytest.mark.parametrize("nparts,rows,channels", BIAS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_reduce_bias_partials(L, nparts, rows, channels, accumulate, kind):
    rng = np.random.default_rng(seed("bias", nparts, rows, channels, accumulate, kind))
    if kind == "exact":
        part = rng.integers(-64, 65, (nparts, rows)).astype(np.float32)
        old = rng.integers(-64, 65, channels).astype(np.float32)
        assert (nparts * (rows // channels) + 1) * 64 < 2 ** 24
    else:
        part, old = rng.standard_normal((nparts, rows)).astype(np.float32), rng.standard_normal(channels).astype(np.float32)
    ref, terms, count = B.reduce_bias_partials(part, channels, old, bool(accumulate))
    pd = f32dev(part)
    first = None
    for _ in range(5):                                            # one thread per channel, slabs in order: the same bits
        out = Out((channels,), torch.float32)
        if accumulate:
            out.t.copy_(torch.from_numpy(old))
        L.check(L.lib().oct_reduce_bias_partials(P(pd), nparts, rows, channels, out.ptr(), accumulate, st()))
        got = out.host()
        if first is None:
            first = got
            if kind == "exact":
                same(got, ref, "reduce_bias_partials (integers)")
            else:
                reduced(got, ref, terms, count, "f32", "reduce_bias_partials")
        else:
            same(got, first, "reduce_bias_partials, repeated")


# ------------------------------------------------------------------------------------------------------------------
# oct_sgd_step and FusedSGD
# ------------------------------------------------------------------------------------------------------------------
def sgd_bounds(p, g, buf, lr, momentum, wd, gscale, first):
    """The kernel rounds four times: g * grad_scale, fma(wd, p, .), fma(momentum, buf, .) and the fused p - lr * (.).  Three of
    them reach buf, all four reach p (the first three scaled by lr <= 1): ulps of the largest intermediate."""
    assert 0 < lr <= 1
    pn, bn, mags = B.sgd_step(p, g, buf, lr, momentum, wd, gscale, first)
    m_b = np.maximum(mags, 0 if bn is None else np.abs(bn))
    m_p = np.maximum.reduce([m_b, np.abs(np.asarray(p, np.float64)), np.abs(pn)])
    return pn, bn, 4 * ulp(m_p, "f32"), 3 * ulp(m_b, "f32")


SGD = [(n, wd, mom, gs, first) for n in (1, 255, 256, 257, 2048 * 256 + 3) for wd in (0.0, 1e-2) for mom in (0.0, 0.9)
       for gs in (1.0, 0.125) for first in (0, 1)]


@pytest.mark.parametrize("n,wd,momentum,gscale,first", SGD)
def test_sgd_step(L, n, wd, momentum, gscale, first):
    lib = L.lib()
    rng = np.random.default_rng(seed("sgd", n, wd, momentum, gscale, first))
    f = lambda v: float(np.float32(v))                                        # noqa: E731
    lr, wd, momentum = f(0.05), f(wd), f(momentum)
    for kind in ("random", "exact"):
        if kind == "exact":                                       # dyadic inputs, power-of-two hyper-parameters: bit-equal
            p, g, b = (rng.integers(-64, 65, n) / 8.0 for _ in range(3))
            hp = (0.125, 0.5 if momentum else 0.0, 2.0 ** -6 if wd else 0.0)
        else:
            p, g, b = (rng.standard_normal(n).astype(np.float32).astype(np.float64) for _ in range(3))
            hp = (lr, momentum, wd)
        pd, bd = Out((n,), torch.float32), Out((n,), torch.float32)
        pd.t.copy_(torch.from_numpy(p.astype(np.float32)))
        if hp[1]:
            bd.t.copy_(torch.from_numpy(b.astype(np.float32)))
        L.check(lib.oct_sgd_step(pd.ptr(), P(f32dev(g)), bd.ptr() if hp[1] else None, n, hp[0], hp[1], hp[2], gscale, first, st()))
        pn, bn, tol_p, tol_b = sgd_bounds(p, g, b if hp[1] else None, hp[0], hp[1], hp[2], gscale, first)
        gp = pd.host()
        if kind == "exact":
            same(gp, pn, "sgd parameters (dyadic operands)")
        else:
            assert (np.abs(gp - pn) <= tol_p).all(), f"sgd parameters: {np.abs(gp - pn).max():.3e}"
        if hp[1]:
            gb = bd.host()
            if kind == "exact":
                same(gb, bn, "sgd momentum buffer (dyadic operands)")
            else:
                assert (np.abs(gb - bn) <= tol_b).all(), f"sgd momentum buffer: {np.abs(gb - bn).max():.3e}"
        else:
            assert bool(torch.isnan(bd.buf).all()), "momentum = 0 leaves buf alone"


@pytest.mark.parametrize("momentum,wd", [(0.9, 1e-2), (0.0, 1e-2), (0.9, 0.0)])
def test_fused_sgd_against_torch_sgd_in_float64(L, momentum, wd):
    """three steps of a small U-Net: FusedSGD on the flat fp32 buffer against torch.optim.SGD on a float64 copy fed the same
    gradients.  The per-step rounding bound compounds: E_b' = mom E_b + wd E_p + 3 ulp, E_p' = E_p + lr (mom E_b + wd E_p) + 4 ulp."""
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    torch.manual_seed(3)
    model = UNet(1, 4, init_features=8, compute_dtype="f32").cuda().train()
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 32, 48, generator=gen).cuda()
    t = torch.randint(0, 4, (2, 32, 48), generator=gen).cuda()
    lr = 0.05
    opt = FusedSGD(list(model.named_parameters()), lr=lr, momentum=momentum, weight_decay=wd)
    lay = opt.layout
    pad = np.ones(lay.total, bool)
    for p, o in zip(lay.params, lay.offsets):
        pad[o:o + p.numel()] = False
    assert pad.any(), "no alignment padding in this model"
    f = lambda v: float(np.float32(v))                                        # noqa: E731
    ref = opt.flat_p.detach().double().cpu().requires_grad_(True)
    topt = torch.optim.SGD([ref], lr=f(lr), momentum=f(momentum), weight_decay=f(wd))
    e_p, e_b = np.zeros(lay.total), np.zeros(lay.total)
    for step in range(3):
        model.forward_backward(x, t, 1.0, 0.5)
        torch.cuda.synchronize()
        g = opt.flat_g.detach().double().cpu()
        assert float(g.abs().sum()) > 0 and not g.numpy()[pad].any()
        p_before = ref.detach().numpy().copy()
        b_before = topt.state[ref]["momentum_buffer"].numpy().copy() if momentum and step else None
        ref.grad = g.clone()
        topt.step()
        opt.step()
        torch.cuda.synchronize()
        _, _, tol_p, tol_b = sgd_bounds(p_before, g.numpy(), b_before, f(lr), f(momentum), f(wd), 1.0, step == 0)
        carried = f(momentum) * e_b + f(wd) * e_p                # the error the step inherits; tol_* are its own roundings
        e_b, e_p = carried + tol_b, e_p + f(lr) * carried + tol_p
        got = opt.flat_p.double().cpu().numpy()
        want = ref.detach().numpy()
        assert (np.abs(got - want) <= e_p).all(), f"step {step}: {np.abs(got - want).max():.3e} > bound"
        assert not got[pad].any(), "the alignment padding of flat_p must stay zero"
        if momentum:
            assert not opt.buf.cpu().numpy()[pad].any()
    assert np.abs(want - p_before).max() > 1e-4, "the parameters did not move"
