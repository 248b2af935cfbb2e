"""The streaming kernels of csrc/blocks.hip and oct_channel_sum (csrc/bn.hip) through the C ABI, against the float64
restatements of oracle/ref_stream.py (themselves pinned to torch by tests/test_oracle_stream.py).

* Selection / copy kernels are compared bit for bit, on integer-valued data (ties) with NaN inside windows.
* One-rounding kernels: the float64 result rounded once to the storage type.  bf16: >= 99.9 % equal (one element may
  differ in a tensor of fewer than 1000), every element within
  1 bf16 ulp (+ 4 * 2^-24 * sum|terms| where fp32 cancels); f32: within max(4 ulp, 4 * 2^-24 * sum|terms|).
* Reductions: |got - ref| <= n * 2^-24 * sum|terms| per output (+ 1 ulp of a bf16 store); a kernel that gathers or promises
  a fixed summation order gives the same bits on five calls.
Every output lands in a buffer longer than the output, filled with NaN (or a sentinel): the tail must survive.  Channel
counts run both vector widths (8 channels per thread when c % 8 == 0, else 1); one case per kernel and dtype has more
than 2.5 * 2^20 work items (the grid is capped at 4096 x 256 = 2^20 threads) and a last pass that is not a multiple of 256.
"""
import numpy as np
import pytest
import torch

from oracle import ref_stream as R
from oracle.bounds import PAD, U, _LIVE, Out, one_rounding, reduced, same, seed, stored, ulp  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
CH = [1, 3, 8, 24, 64, 512]
N_, H_, W_ = 2, 7, 11           # odd / prime spatial sizes
BIG = (2, 1031, 1283)           # n * h * w = 2,645,546 pixels: 2.52 * 2^20, 42 past a multiple of 256


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    _lib.lib()
    return _lib


def tdt(dt):
    return torch.float32 if dt == "f32" else torch.bfloat16


def dcode(L, dt):
    return L.DT_F32 if dt == "f32" else L.DT_BF16


def st():
    return torch.cuda.current_stream().cuda_stream


# device inputs live until the test ends (see oracle/bounds.py)
@pytest.fixture(autouse=True)
def _keep_inputs_alive():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def todev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to("cuda", tdt(dt))
    _LIVE.append(t)
    return t


def f32dev(a):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()
    _LIVE.append(t)
    return t


def shapes(big_c=8):
    return [(N_, H_, W_, c) for c in CH] + [BIG + (big_c,)]


def sid(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------------------------------------------
# affine + activation (+ residual, + the residual's deferred bias)
# ------------------------------------------------------------------------------------------------------------------
CASES_AFFINE = [(s, act, rm) for s in shapes()[:-1] for act in (0, 1, 2) for rm in ("none", "res", "res_shift")] + \
               [(BIG + (8,), 2, "res_shift"), (BIG + (8,), 1, "res")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,act,rm", CASES_AFFINE, ids=[f"{sid(s)}-act{a}-{r}" for s, a, r in CASES_AFFINE])
def test_affine_act_fwd(L, dt, shape, act, rm):
    n, h, w, c = shape
    rng = np.random.default_rng(seed(shape, act, rm, dt))
    y = stored(rng.standard_normal(shape) * 3, dt)
    sc = (rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c)).astype(np.float32)
    sh = (rng.standard_normal(c) * 0.5).astype(np.float32)
    sh[0] = 0.0
    y[..., 0].flat[::5] = 0.0                                 # z == 0 exactly
    res = stored(rng.standard_normal(shape), dt) if rm != "none" else None
    rb = (rng.standard_normal(c) * 0.5).astype(np.float32) if rm == "res_shift" else None
    out = Out(shape, tdt(dt))
    L.check(L.lib().oct_affine_res_act_fwd(dcode(L, dt), todev(y, dt).data_ptr(), f32dev(sc).data_ptr(), f32dev(sh).data_ptr(),
                                           None if res is None else todev(res, dt).data_ptr(), None if rb is None else f32dev(rb).data_ptr(),
                                           act, out.ptr(), n * h * w, c, st()), "oct_affine_res_act_fwd")
    ref, terms, z = R.affine_act(y, sc, sh, act, res, rb, store=lambda v: stored(v, dt))
    if act == R.ACT_SIGMOID:   # error in z damped by sigma' <= 1/4; __expf: relative error ~ (|z| + 2) 2^-24
        terms = terms * ref * (1 - ref) + ref * (np.abs(z) + 4)
    one_rounding(out.host(), ref, terms, dt, f"affine_act act={act} {rm}")


def test_affine_act_fwd_without_residual_entry_point(L):
    rng = np.random.default_rng(1)
    n, h, w, c = N_, H_, W_, 24
    y = stored(rng.standard_normal((n, h, w, c)), "bf16")
    sc, sh = np.ones(c, np.float32), rng.standard_normal(c).astype(np.float32)
    out = Out((n, h, w, c), torch.bfloat16)
    L.check(L.lib().oct_affine_act_fwd(L.DT_BF16, todev(y, "bf16").data_ptr(), f32dev(sc).data_ptr(), f32dev(sh).data_ptr(), None,
                                       L.ACT_RELU, out.ptr(), n * h * w, c, st()))
    ref, terms, _ = R.affine_act(y, sc, sh, R.ACT_RELU)
    one_rounding(out.host(), ref, terms, "bf16", "affine_act_fwd")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", [1, 3, 8, 24, 64])
@pytest.mark.parametrize("entry", ["act", "res", "res_shift"])
def test_affine_relu_keeps_nan(L, dt, c, entry):
    """torch.relu(NaN) is NaN: the output is NaN exactly where relu(y*scale + shift (+ res)) in float64 is, also through a NaN
    scale; elsewhere nothing changes"""
    n, h, w = N_, H_, W_
    shape = (n, h, w, c)
    rng = np.random.default_rng(seed("nan", c, entry, dt))
    y = stored(rng.standard_normal(shape) * 3, dt)
    y[0, 0, 0, 0] = y[0, 3, 4, min(7, c - 1)] = y[-1, h - 1, w - 1, c - 1] = y[-1, 2, 2, (c // 2 // 8) * 8] = np.nan
    sc = (rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c)).astype(np.float32)
    sh = (rng.standard_normal(c) * 0.5).astype(np.float32)
    res = stored(rng.standard_normal(shape), dt) if entry != "act" else None
    rb = (rng.standard_normal(c) * 0.5).astype(np.float32) if entry == "res_shift" else None
    if res is not None:
        res[0, 1, 1, c - 1] = np.nan                              # a NaN residual reaches the output too
    for nan_scale in ((False, True) if c > 1 else (False,)):
        s = sc.copy()
        if nan_scale:
            s[c // 2] = np.nan
        with np.errstate(invalid="ignore"):
            z = y * s.astype(np.float64) + sh.astype(np.float64) + (0 if res is None else res + (0 if rb is None else rb.astype(np.float64)))
        want = torch.relu(torch.from_numpy(z)).numpy()
        assert np.isnan(want).sum() >= 3 and not np.isnan(want).all()
        out = Out(shape, tdt(dt))
        if entry == "act":
            L.check(L.lib().oct_affine_act_fwd(dcode(L, dt), todev(y, dt).data_ptr(), f32dev(s).data_ptr(), f32dev(sh).data_ptr(), None,
                                               L.ACT_RELU, out.ptr(), n * h * w, c, st()))
        else:
            L.check(L.lib().oct_affine_res_act_fwd(dcode(L, dt), todev(y, dt).data_ptr(), f32dev(s).data_ptr(), f32dev(sh).data_ptr(),
                                                   todev(res, dt).data_ptr(), None if rb is None else f32dev(rb).data_ptr(),
                                                   L.ACT_RELU, out.ptr(), n * h * w, c, st()))
        got = out.host()
        assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN where torch.relu has NaN, nowhere else"
        ok = ~np.isnan(want)
        clean = lambda a: None if a is None else np.where(np.isnan(a), 0.0, a)          # noqa: E731
        ref, terms, _ = R.affine_act(clean(y), np.where(np.isnan(s), 1.0, s), sh, R.ACT_RELU, clean(res), rb, store=lambda v: stored(v, dt))
        one_rounding(np.where(ok, got, 0.0), np.where(ok, ref, 0.0), terms, dt, f"affine relu ({entry}) away from the NaNs")


# act_bwd picks its vector width from the element count: 154 * c is a multiple of 8 only for c % 8 == 0 here
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", shapes(), ids=sid)
@pytest.mark.parametrize("act", [1, 2])
def test_act_bwd(L, dt, shape, act):
    rng = np.random.default_rng(seed(shape, act, dt))
    z = rng.standard_normal(shape) * 2
    o = stored(np.maximum(z, 0) if act == 1 else 1 / (1 + np.exp(-z)), dt)
    assert act == 2 or (o == 0).any()
    d = stored(rng.standard_normal(shape), dt)
    out = Out(shape, tdt(dt))
    L.check(L.lib().oct_act_bwd(dcode(L, dt), todev(d, dt).data_ptr(), todev(o, dt).data_ptr(), act, out.ptr(), d.size, st()))
    ref = R.act_bwd(d, o, act)
    if act == 1:
        same(out.host(), ref, "relu backward")
    else:
        one_rounding(out.host(), ref, np.abs(ref), dt, "sigmoid backward")


# ------------------------------------------------------------------------------------------------------------------
# max-pooling family: bit equality, ties to the first maximum, NaN propagates (the last NaN of the window wins)
# ------------------------------------------------------------------------------------------------------------------
def pool_input(rng, shape, dt):
    a = rng.integers(-3, 4, shape).astype(np.float32)
    n, h, w, c = shape
    a[0, 0, 1, 0] = np.nan
    a[0, 1, 0, 0] = np.nan
    a[-1, h - 1, w - 1, c - 1] = np.nan
    a[-1, 2, 3, c // 2] = np.nan
    return a


POOL = [(N_, H_, W_, c, k) for c in CH for k in (2, 3)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", POOL, ids=sid)
def test_maxpool_fwd_bwd(L, dt, shape):
    n, h, w, c, k = shape
    rng = np.random.default_rng(seed(shape, dt))
    a = pool_input(rng, (n, h, w, c), dt)
    ad = todev(a, dt)
    ref, code = R.maxpool(a, k)
    out = Out(ref.shape, tdt(dt))
    L.check(L.lib().oct_maxpool_fwd(dcode(L, dt), ad.data_ptr(), out.ptr(), n, h, w, c, k, st()))
    got = out.host()
    assert np.isnan(ref).any()
    same(got, ref, "maxpool forward")
    dout = rng.integers(1, 9, ref.shape).astype(np.float32)
    da = Out((n, h, w, c), tdt(dt))
    L.check(L.lib().oct_maxpool_bwd(dcode(L, dt), ad.data_ptr(), todev(dout, dt).data_ptr(), da.ptr(), n, h, w, c, k, st()))
    same(da.host(), R.window_scatter(dout, code, k, h, w), "maxpool backward")


def _pool_family(L, dt, a, k, rng):
    """maxpool_idx_fwd + index scatter / gather and maxpool_code_fwd + window scatter / gather on one input (h, w multiples of k)"""
    lib = L.lib()
    n, h, w, c = a.shape
    hp, wp = h // k, w // k
    ad = todev(a, dt)
    ref, code = R.maxpool(a, k)
    pidx = R.maxpool_plane_index(code, k, w)
    out, idx = Out(ref.shape, tdt(dt)), Out(ref.shape, torch.int64, fill=-7)
    L.check(lib.oct_maxpool_idx_fwd(dcode(L, dt), ad.data_ptr(), out.ptr(), idx.ptr(), n, h, w, c, k, st()))
    same(out.host(), ref, "maxpool_idx_fwd value")
    same(idx.host(), pidx, "maxpool_idx_fwd index (torch's per-plane iy*W + ix)")
    out2, cd = Out(ref.shape, tdt(dt)), Out(ref.shape, torch.uint8, fill=0xEE)
    L.check(lib.oct_maxpool_code_fwd(dcode(L, dt), ad.data_ptr(), out2.ptr(), cd.ptr(), n, h, w, c, k, st()))
    same(out2.host(), ref, "maxpool_code_fwd value")
    same(cd.host(), code, "maxpool_code_fwd window code")
    v = rng.integers(1, 9, ref.shape).astype(np.float32)
    vd = todev(v, dt)
    # index scatter (MaxUnpool2d): the caller zero-fills; indices outside the plane are skipped
    qi = pidx.copy()
    qi[0, 0, 0, 0], qi[-1, -1, -1, -1] = -1, h * w
    qd = torch.from_numpy(qi).cuda()
    sc = Out((n, h, w, c), tdt(dt))
    sc.t.zero_()
    L.check(lib.oct_index_scatter(dcode(L, dt), vd.data_ptr(), qd.data_ptr(), sc.ptr(), n, hp * wp, h * w, c, st()))
    same(sc.host(), R.index_scatter(v, qi, h, w), "index_scatter")
    x = stored(rng.standard_normal((n, h, w, c)), dt)
    xd = todev(x, dt)
    ga = Out(ref.shape, tdt(dt))
    L.check(lib.oct_index_gather(dcode(L, dt), xd.data_ptr(), qd.data_ptr(), ga.ptr(), n, hp * wp, h * w, c, st()))
    same(ga.host(), R.index_gather(x, qi), "index_gather")
    cdd = torch.from_numpy(code.astype(np.uint8)).cuda()
    ws = Out((n, h, w, c), tdt(dt))                            # dense: no fill needed
    L.check(lib.oct_window_scatter(dcode(L, dt), vd.data_ptr(), cdd.data_ptr(), ws.ptr(), n, hp, wp, c, k, st()))
    same(ws.host(), R.window_scatter(v, code, k), "window_scatter")
    wg = Out(ref.shape, tdt(dt))
    L.check(lib.oct_window_gather(dcode(L, dt), xd.data_ptr(), cdd.data_ptr(), wg.ptr(), n, hp, wp, c, k, st()))
    same(wg.host(), R.window_gather(x, code, k), "window_gather")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", CH)
@pytest.mark.parametrize("k", [2, 3])
def test_maxpool_index_and_window_code_family(L, dt, c, k):
    rng = np.random.default_rng(seed(c, k, dt))
    _pool_family(L, dt, pool_input(rng, (N_, H_ * k, W_ * k, c), dt), k, rng)


@pytest.mark.parametrize("dt", DTYPES)
def test_pooling_grid_stride_tail(L, dt):
    """2.5 * 2^20 pooled outputs (one channel: the input stays 10.6 M elements) through every pooling kernel"""
    rng = np.random.default_rng(11)
    n, hp, wp = BIG
    a = pool_input(rng, (n, 2 * hp, 2 * wp, 1), dt)
    ad = todev(a, dt)
    ref, code = R.maxpool(a, 2)
    out = Out(ref.shape, tdt(dt))
    L.check(L.lib().oct_maxpool_fwd(dcode(L, dt), ad.data_ptr(), out.ptr(), n, 2 * hp, 2 * wp, 1, 2, st()))
    same(out.host(), ref, "maxpool forward")
    dout = rng.integers(1, 9, ref.shape).astype(np.float32)
    da = Out(a.shape, tdt(dt))
    L.check(L.lib().oct_maxpool_bwd(dcode(L, dt), ad.data_ptr(), todev(dout, dt).data_ptr(), da.ptr(), n, 2 * hp, 2 * wp, 1, 2, st()))
    same(da.host(), R.window_scatter(dout, code, 2), "maxpool backward")
    _pool_family(L, dt, a, 2, rng)


DEPTH = [(3, m) for m in (1, 3, 8, 24, 64, 77 * 8, 1001)] + [(BIG[0], BIG[1] * BIG[2] * 8)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nslab,m", DEPTH)
def test_depth_pool(L, dt, nslab, m):
    rng = np.random.default_rng(nslab * 7 + m)
    p2 = rng.integers(-2, 3, (nslab, 2, m)).astype(np.float32)     # ties between the slices
    p2[0, 1, 0] = np.nan
    p2[-1, 0, m - 1] = np.nan
    p2[-1, :, m // 2] = np.nan
    ref, _ = R.depth_pool(p2)
    pd = todev(p2, dt)
    out = Out(ref.shape, tdt(dt))
    L.check(L.lib().oct_depth_pool_fwd(dcode(L, dt), pd.data_ptr(), out.ptr(), nslab, m, st()))
    same(out.host(), ref, "depth_pool_fwd")
    d = rng.integers(1, 9, ref.shape).astype(np.float32)
    dp = Out(p2.shape, tdt(dt))
    L.check(L.lib().oct_depth_pool_bwd(dcode(L, dt), pd.data_ptr(), todev(d, dt).data_ptr(), dp.ptr(), nslab, m, st()))
    same(dp.host(), R.depth_pool_bwd(p2, d), "depth_pool_bwd")


# ------------------------------------------------------------------------------------------------------------------
# bilinear resize, align_corners=True
# ------------------------------------------------------------------------------------------------------------------
BIL = [(7, 11, 13, 21), (13, 21, 7, 11), (1, 11, 3, 21), (7, 11, 1, 5), (7, 1, 9, 1), (7, 11, 7, 11), (31, 5, 62, 10),
       (62, 3, 124, 6), (124, 3, 248, 6), (9, 13, 4, 29)]


def _bilinear(L, dt, n, h, w, c, ho, wo, factor=None):
    lib = L.lib()
    rng = np.random.default_rng(seed(h, w, c, ho, wo, dt))
    x = stored(rng.standard_normal((n, h, w, c)), dt)
    out = Out((n, ho, wo, c), tdt(dt))
    if factor:
        L.check(lib.oct_bilinear_up_fwd(dcode(L, dt), todev(x, dt).data_ptr(), out.ptr(), n, h, w, c, factor, st()))
    else:
        L.check(lib.oct_bilinear_resize_fwd(dcode(L, dt), todev(x, dt).data_ptr(), out.ptr(), n, h, w, c, ho, wo, st()))
    ref, terms = R.bilinear_fwd(x, ho, wo)
    one_rounding(out.host(), ref, terms, dt, f"bilinear {h}x{w} -> {ho}x{wo} forward")
    d = stored(rng.standard_normal((n, ho, wo, c)), dt)
    dd = todev(d, dt)
    ref, terms, count = R.bilinear_bwd(d, h, w)
    runs = []
    for _ in range(5):                                           # a gather: the same bits every call
        dx = Out((n, h, w, c), tdt(dt))
        if factor:
            L.check(lib.oct_bilinear_up_bwd(dcode(L, dt), dd.data_ptr(), dx.ptr(), n, h, w, c, factor, st()))
        else:
            L.check(lib.oct_bilinear_resize_bwd(dcode(L, dt), dd.data_ptr(), dx.ptr(), n, h, w, c, ho, wo, st()))
        runs.append(dx.host())
    reduced(runs[0], ref, terms, 2 * count[None, :, :, None] + 2, dt, f"bilinear {h}x{w} -> {ho}x{wo} backward",
            stored_dt=dt if dt == "bf16" else None)
    for r in runs[1:]:
        same(r, runs[0], "bilinear backward, repeated")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("c", CH)
@pytest.mark.parametrize("size", BIL, ids=sid)
def test_bilinear_resize(L, dt, c, size):
    h, w, ho, wo = size
    _bilinear(L, dt, N_, h, w, c, ho, wo)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("h,w,c,factor", [(31, 48, 8, 2), (62, 5, 3, 2), (7, 11, 64, 4), (5, 3, 24, 1)])
def test_bilinear_up(L, dt, h, w, c, factor):
    _bilinear(L, dt, N_, h, w, c, h * factor, w * factor, factor)


@pytest.mark.parametrize("dt", DTYPES)
def test_bilinear_grid_stride_tail(L, dt):
    n, h, w = BIG
    _bilinear(L, dt, n, (h + 1) // 2, (w + 1) // 2, 8, h, w)     # forward: 2.6 M output pixels
    _bilinear(L, dt, n, h, w, 8, (h + 1) // 2, (w + 1) // 2)     # backward: 2.6 M input pixels (shrinking)


# ------------------------------------------------------------------------------------------------------------------
# depth-to-space / space-to-depth
# ------------------------------------------------------------------------------------------------------------------
D2S = [(N_, H_, W_, c, 2) for c in CH] + [(1, 5, 3, 3, 4), (1, 3, 5, 8, 4), (BIG[0], 516, 642, 8, 2)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", D2S, ids=sid)
def test_depth_to_space_and_back(L, dt, shape):
    n, h, w, cout, s = shape
    lib = L.lib()
    rng = np.random.default_rng(seed(shape, dt))
    x = stored(rng.standard_normal((n, h, w, s * s * cout)), dt)
    xd = todev(x, dt)
    out = Out((n, h * s, w * s, cout), tdt(dt))
    L.check(lib.oct_depth_to_space(dcode(L, dt), xd.data_ptr(), None, out.ptr(), n, h, w, cout, s, st()))
    wide = out.host()
    same(wide, R.depth_to_space(x, s), "depth_to_space")
    back = Out(x.shape, tdt(dt))
    L.check(lib.oct_space_to_depth(dcode(L, dt), todev(wide, dt).data_ptr(), back.ptr(), n, h, w, cout, s, st()))
    same(back.host(), x, "space_to_depth")
    b = rng.standard_normal(cout).astype(np.float32)
    ob = Out((n, h * s, w * s, cout), tdt(dt))
    L.check(lib.oct_depth_to_space(dcode(L, dt), xd.data_ptr(), f32dev(b).data_ptr(), ob.ptr(), n, h, w, cout, s, st()))
    ref = R.depth_to_space(x, s, b)
    one_rounding(ob.host(), ref, np.abs(R.depth_to_space(x, s)) + np.abs(b), dt, "depth_to_space + bias")


# ------------------------------------------------------------------------------------------------------------------
# attention gate product
# ------------------------------------------------------------------------------------------------------------------
GATE = [(N_, H_, W_, c) for c in CH + [128, 520]] + [BIG + (8,)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", GATE, ids=sid)
def test_gate(L, dt, shape):
    n, h, w, c = shape
    npix = n * h * w
    lib = L.lib()
    rng = np.random.default_rng(seed(shape, dt))
    x = stored(rng.standard_normal(shape), dt)
    p = stored(rng.random((n, h, w, 1)), dt)
    xd, pd = todev(x, dt), todev(p, dt)
    out = Out(shape, tdt(dt))
    L.check(lib.oct_gate_fwd(dcode(L, dt), xd.data_ptr(), pd.data_ptr(), out.ptr(), npix, c, st()))
    one_rounding(out.host(), R.gate_fwd(x, p), np.abs(R.gate_fwd(x, p)), dt, "gate forward")
    d = stored(rng.standard_normal(shape), dt)
    dd = todev(d, dt)
    rdx, rdp, tdp = R.gate_bwd(d, x, p)
    dps = []
    for _ in range(5):                                           # fixed shuffle tree / sequential loop: same bits
        dx, dp = Out(shape, tdt(dt)), Out((n, h, w, 1), tdt(dt))
        L.check(lib.oct_gate_bwd(dcode(L, dt), dd.data_ptr(), xd.data_ptr(), pd.data_ptr(), dx.ptr(), dp.ptr(), npix, c, st()))
        if not dps:
            one_rounding(dx.host(), rdx, np.abs(rdx), dt, "gate backward dx")
        dps.append(dp.host())
    reduced(dps[0], rdp, tdp, c, dt, "gate backward dp", stored_dt=dt)
    for r in dps[1:]:
        same(r, dps[0], "gate backward dp, repeated")


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm-apply + PReLU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", shapes(), ids=sid)
def test_affine_prelu(L, dt, shape):
    n, h, w, c = shape
    npix = n * h * w
    lib = L.lib()
    rng = np.random.default_rng(seed(shape, dt))
    y = stored(rng.integers(-8, 9, shape) * 0.25 + rng.standard_normal(shape) * (rng.random(shape) < 0.5), dt)
    sc = (rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c)).astype(np.float32)
    sh = (rng.standard_normal(c) * 0.5).astype(np.float32)
    sc[0], sh[0] = 1.0, 0.0                                      # z == 0 wherever y == 0 in channel 0
    y[..., 0].flat[::7] = 0.0
    alpha = np.array([0.25], np.float32)
    yd, scd, shd, ad = todev(y, dt), f32dev(sc), f32dev(sh), f32dev(alpha)
    out = Out(shape, tdt(dt))
    L.check(lib.oct_affine_prelu_fwd(dcode(L, dt), yd.data_ptr(), scd.data_ptr(), shd.data_ptr(), ad.data_ptr(), out.ptr(), npix, c, st()))
    ref, terms, z = R.affine_prelu(y, sc, sh, alpha[0])
    assert (z == 0).any()
    one_rounding(out.host(), ref, terms, dt, "affine_prelu forward")
    d = stored(rng.standard_normal(shape), dt)
    dz = Out(shape, tdt(dt))
    da = Out((1,), torch.float32)
    da.t.zero_()
    L.check(lib.oct_affine_prelu_bwd(dcode(L, dt), todev(d, dt).data_ptr(), yd.data_ptr(), scd.data_ptr(), shd.data_ptr(), ad.data_ptr(),
                                     dz.ptr(), da.ptr(), npix, c, st()))
    # the kernel recomputes z = fma(y, scale, shift): z rounded once to fp32 (same sign, z == 0 stays exact)
    rdz, rda, tda = R.affine_prelu_bwd(d, z.astype(np.float32), alpha[0])
    one_rounding(dz.host(), rdz, np.abs(rdz), dt, "affine_prelu backward dz")
    # dalpha: global fp32 atomics (no order promised): the bound only
    reduced(da.host(), np.array([rda]), np.array([tda]), npix * c, dt, "affine_prelu backward dalpha")


# ------------------------------------------------------------------------------------------------------------------
# 1x1 convolution with K outputs: weight / bias gradient (fixed summation order), and oct_channel_sum
# ------------------------------------------------------------------------------------------------------------------
ROWDOT = [(3 * 37 * 53 + 1, c, k) for c, k in ((8, 1), (64, 3), (512, 4), (16, 9), (64, 10), (128, 12))] + \
         [(BIG[0] * BIG[1] * BIG[2], c, k) for c, k in ((8, 1), (64, 10))]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("npix,c,k", ROWDOT)
def test_rowdot_weight_and_bias_gradients_random_data(L, dt, npix, c, k):
    lib = L.lib()
    rng = np.random.default_rng(c * 100 + k + npix)
    x = stored(rng.standard_normal((npix, c)), dt)
    dy = stored(rng.standard_normal((npix, k)), dt)
    xd, dyd = todev(x, dt), todev(dy, dt)
    nblk = lib.oct_rowdot_blocks(npix, c)
    rdw, rdb, tdw, tdb = R.rowdot_bwd_weight(dy, x)
    dws, dbs = [], []
    for _ in range(5):
        part = torch.empty((nblk, k * c + k), dtype=torch.float32, device="cuda")
        dw, db = Out((k, c), torch.float32), Out((k,), torch.float32)
        L.check(lib.oct_rowdot_bwd_weight_bias(dcode(L, dt), dyd.data_ptr(), xd.data_ptr(), dw.ptr(), db.ptr(), part.data_ptr(),
                                               npix, c, k, 0, st()))
        dws.append(dw.host())
        dbs.append(db.host())
    reduced(dws[0], rdw, tdw, npix, dt, "rowdot dw")
    reduced(dbs[0], rdb, tdb, npix, dt, "rowdot dbias")
    for a, b in zip(dws[1:], dbs[1:]):
        same(a, dws[0], "rowdot dw, repeated")
        same(b, dbs[0], "rowdot dbias, repeated (the kernel promises a fixed summation order)")
    part = torch.empty((nblk, k * c), dtype=torch.float32, device="cuda")
    dw = Out((k, c), torch.float32)
    L.check(lib.oct_rowdot_bwd_weight(dcode(L, dt), dyd.data_ptr(), xd.data_ptr(), dw.ptr(), part.data_ptr(), npix, c, k, 0, st()))
    same(dw.host(), dws[0], "dw without the bias riding on the pass")


CSUM = [(N_ * H_ * W_, c) for c in CH] + [(1001, 40), (BIG[0] * BIG[1] * BIG[2], 8), (BIG[0] * BIG[1] * BIG[2] // 4, 3)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("npix,c", CSUM)
def test_channel_sum(L, dt, npix, c):
    """flat kernel (c % 8 == 0, c / 8 a power of two) and element kernel (any other c), accumulate 0 and 1: fp32 atomics,
    no order promised -- the bound on random data, exact sums on integer data"""
    lib = L.lib()
    rng = np.random.default_rng(npix + c)
    x = stored(rng.standard_normal((npix, c)) + np.arange(c), dt)
    xd = todev(x, dt)
    ref, terms = R.channel_sum(x)
    out = Out((c,), torch.float32)
    out.t.fill_(123.0)
    L.check(lib.oct_channel_sum(dcode(L, dt), xd.data_ptr(), out.ptr(), npix, c, 0, st()))
    reduced(out.host(), ref, terms, npix, dt, "channel_sum")
    L.check(lib.oct_channel_sum(dcode(L, dt), xd.data_ptr(), out.ptr(), npix, c, 1, st()))
    reduced(out.host(), 2 * ref, 2 * terms, 2 * npix, dt, "channel_sum accumulate")
    xi = rng.integers(-2, 3, (npix, c)).astype(np.float32)     # |partial sums| < 2^24: exact in any order
    xi[:, -1] = 1.0
    L.check(lib.oct_channel_sum(dcode(L, dt), todev(xi, dt).data_ptr(), out.ptr(), npix, c, 0, st()))
    same(out.host(), xi.astype(np.float64).sum(0), "channel_sum of integers")
