"""oct_conv_backward_fused (igemm2.hip, FUSE): the backward of a 32 -> 32 convolution fed by relu(bn(y1)) in ONE launch --
the data gradient dA1, the weight gradient and the BatchNorm-backward partial sums of the layer below.

* exact operands (the method of tests/test_gpu_exact.py): every sum is exact in fp32 in any order, so dX, dW and the column
  totals of the partial rows must equal the float64 reference BIT FOR BIT;
* random bf16 operands: dX bit-identical to the data-gradient launch it replaces, the partial rows within the bound of
  tests/test_gpu_bn.py::test_dact_bn_reduce, dW no further from float64 than twice oct_conv_wgrad's own error;
* two launches give the same dX and the same partial rows; descriptors the kernel does not take are refused untouched;
* one bf16 training step of the wide fixture with and without the fused launches.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ref_bn as B
from oracle import ref_cpu as O
from oracle.bounds import reduced

pytestmark = pytest.mark.gpu

# (n, h, w): tiles side by side | stacked, top and bottom padding | a tile with neighbours on all sides |
# >= 512 tiles: the interleaved walk, several tiles per workgroup | 600 tiles: the interleaved walk with unequal tile counts
# (88 workgroups take three tiles, 168 take two)
SHAPES = [(2, 16, 64), (1, 32, 32), (1, 48, 96), (16, 64, 256), (3, 80, 640)]
CH = 32


@pytest.fixture(scope="module")
def env():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    from retinal_oct_image_segmentation_via_deep_learning_amd import engine as E
    L.lib()
    return L, E


def to_bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def dev(a_nchw):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a_nchw, np.float32).transpose(0, 2, 3, 1))).to("cuda", torch.bfloat16)


def host(t_nhwc):
    return t_nhwc.float().cpu().numpy().transpose(0, 3, 1, 2)


def fdev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda().contiguous()


def same(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    bad = got != ref
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                           f"{np.unravel_index(bad.argmax(), bad.shape)}: got {got[bad][0]!r} want {ref[bad][0]!r}")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))


def bc(v):
    return np.asarray(v, np.float64)[None, :, None, None]


def desc(L, n, h, w, dt=None, c0=CH, c1=0, cout=CH, xf=None, partials=0):
    return L.WgradDesc(L.DT_BF16 if dt is None else dt, n, h, w, c0, c1, cout, 9, L.XF_AFFINE_RELU if xf is None else xf, L.XF_NONE,
                       L.IN_PLAIN, 0, 0, 0, 0, 0, 0, partials)


def st():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """device operands of one layer (uploaded once) and what a launch returns"""

    def __init__(self, L, E, n, h, w, y1, sc, sh, mu, inv, dy, wt):
        self.L, self.n, self.h, self.w = L, n, h, w
        self.y1, self.dy = dev(y1), dev(dy)
        self.vec = [fdev(v) for v in (sc, sh, mu, inv)]
        self.wt = fdev(wt)
        self.eng = E.UNetEngine(1, 2, 4, "bf16")
        self.wp = self.eng._pack("w", self.wt, L.PACK_CONV_DGRAD, CH, CH)
        self.bn = E.BNState(*self.vec)
        self.E = E

    def launch(self):
        """-> dX (n, c, h, w), dW (cout, cin, 3, 3), partial rows (blocks, 2, c), all on the host"""
        L, n, h, w = self.L, self.n, self.h, self.w
        lib = L.lib()
        d = desc(L, n, h, w)
        assert lib.oct_conv_backward_fused_ok(C.byref(d)) == 1
        nb = lib.oct_conv_backward_fused_blocks(C.byref(d))
        assert 1 <= nb <= 256
        dx = torch.full((n, h, w, CH), float("nan"), dtype=torch.bfloat16, device="cuda")
        parts = torch.full((nb, 2, CH), float("nan"), dtype=torch.float32, device="cuda")
        dwp = torch.zeros((9, CH, CH), dtype=torch.float32, device="cuda")
        a = L.ConvBwdFusedArgs(self.y1.data_ptr(), *[v.data_ptr() for v in self.vec], self.dy.data_ptr(), self.wp.data_ptr(),
                               dx.data_ptr(), dwp.data_ptr(), parts.data_ptr())
        L.check(lib.oct_conv_backward_fused(C.byref(d), C.byref(a), st()), "oct_conv_backward_fused")
        grad = torch.full((CH, CH, 3, 3), float("nan"), dtype=torch.float32, device="cuda")
        L.check(lib.oct_unpack_wgrad(L.PACK_CONV_FPROP, dwp.data_ptr(), grad.data_ptr(), CH, CH, 0, st()), "oct_unpack_wgrad")
        torch.cuda.synchronize()
        return dx, grad.cpu().numpy(), parts.cpu().numpy()

    def separate(self):
        """the launches the fused one replaces: (dX device tensor, dW host)"""
        L, E, n, h, w = self.L, self.E, self.n, self.h, self.w
        dx = torch.full((n, h, w, CH), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.eng._conv(E.Src(self.dy, CH), self.wp, CH, 9, n, h, w, dx)
        dwp = self.eng._wgrad(E.Src(self.y1, CH, self.bn), self.dy, CH, 9, n, h, w)
        grad = torch.full((CH, CH, 3, 3), float("nan"), dtype=torch.float32, device="cuda")
        self.eng._unpack(L.PACK_CONV_FPROP, dwp, grad, CH, CH, False)
        torch.cuda.synchronize()
        return dx, grad.cpu().numpy()


# ---- exact operands -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(shape):
    """Host operands and the float64 reference of one shape, computed once.  y1: integers in [-4, 4]; scale in {+-0.5, +-1, 2},
    shift in halves + 0.25 (no tie at the mask); mean in halves, invstd a power of two; dY: integers in [-2, 2] at ~50 %
    density; weights 0 or +-2^k.  x = relu(y1*scale + shift) is a multiple of 0.25 below 16 (exact in bf16), dX a multiple of
    the smallest weight, xhat a multiple of 0.5 * invstd.  The large shape thins dY and the weights and keeps the weights and
    invstd at >= 0.5 / >= 1, so that its 262144-term sums stay below 2^24 granules (so do the 68096-term sums of the contiguous-walk
    shapes of tests/test_gpu_tile_walk.py, which trip the guards below with the denser operands)."""
    n, h, w = shape
    big = n * h * w > 50000
    rng = np.random.default_rng(1000 + n * 7 + h * 3 + w)
    y1 = rng.integers(-4, 5, (n, CH, h, w)).astype(np.float64)
    sc = rng.choice([-1.0, -0.5, 0.5, 1.0, 2.0], CH)
    sh = rng.integers(-2, 3, CH) * 0.5 + 0.25
    mu = rng.integers(-2, 3, CH) * 0.5
    inv = rng.choice([1.0, 2.0] if big else [0.5, 1.0, 2.0], CH)
    dy = rng.integers(-2, 3, (n, CH, h, w)) * (rng.random((n, CH, h, w)) < (0.1 if big else 0.5))
    dy = dy.astype(np.float64)
    kmin = -1 if big else -3
    wt = np.exp2(rng.integers(kmin, 1, (CH, CH, 3, 3))) * rng.choice([-1.0, 1.0], (CH, CH, 3, 3)) * \
        (rng.random((CH, CH, 3, 3)) < (0.15 if big else 0.6))
    z = y1 * bc(sc) + bc(sh)
    assert (z != 0).all()                                     # no tie at the mask
    x = np.maximum(z, 0.0)
    assert np.array_equal(to_bf16(x), x)
    dx, dw = O.conv3x3_bwd(x, wt, dy)
    g = np.where(z > 0, to_bf16(dx).astype(np.float64), 0.0)   # dA1 as stored
    xhat = (y1 - bc(mu)) * bc(inv)
    gx = g * xhat
    # the premise, on the float64 reference: every partial sum, in any order, is an integer number of granules below 2^24
    # (granule: dX 2^kmin; g after the bf16 store is a multiple of it too; xhat 0.5 * min invstd; x 0.25; dY 1)
    gran_dx = 2.0 ** kmin
    gran_gx = gran_dx * 0.5 * inv.min()
    assert np.abs(dx).max() * 2 / gran_dx < 2 ** 24
    assert np.abs(dw).max() * 2 / 0.25 < 2 ** 24
    assert np.abs(g).sum(axis=(0, 2, 3)).max() * 2 / gran_dx < 2 ** 24
    assert np.abs(gx).sum(axis=(0, 2, 3)).max() * 2 / gran_gx < 2 ** 24
    # dW: the largest sum of |terms| of one output (a bound on every partial sum of it)
    ax = np.abs(x)
    ady = np.abs(dy)
    assert ady.sum(axis=(0, 2, 3)).max() * ax.max() * 2 / 0.25 < 2 ** 24
    return dict(y1=y1, sc=sc, sh=sh, mu=mu, inv=inv, dy=dy, wt=wt, dx=dx, dw=dw, s1=g.sum(axis=(0, 2, 3)), s2=gx.sum(axis=(0, 2, 3)))


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_backward_bit_exact(env, shape):
    L, E = env
    n, h, w = shape
    r = exact_case(shape)
    case = Case(L, E, n, h, w, r["y1"], r["sc"], r["sh"], r["mu"], r["inv"], r["dy"], r["wt"])
    dx, dw, parts = case.launch()
    same(host(dx), to_bf16(r["dx"]), "dX (bf16 store of the exact sum)")
    same(dw, r["dw"], "dW")
    tot = parts.astype(np.float64).sum(0)
    same(tot[0], r["s1"], "BatchNorm-backward sum g")
    same(tot[1], r["s2"], "BatchNorm-backward sum g * xhat")
    dx_sep, dw_sep = case.separate()
    assert torch.equal(dx.view(torch.int16), dx_sep.view(torch.int16)), "dX differs from the data-gradient launch"
    same(dw, dw_sep, "dW against oct_conv_wgrad")


# ---- random bf16 operands ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(shape):
    n, h, w = shape
    rng = np.random.default_rng(2000 + n * 7 + h * 3 + w)
    y1 = to_bf16(rng.standard_normal((n, CH, h, w))).astype(np.float64)
    dy = to_bf16(rng.standard_normal((n, CH, h, w))).astype(np.float64)
    sc = (rng.uniform(0.5, 1.5, CH) * rng.choice([-1.0, 1.0], CH)).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, CH).astype(np.float32)
    mu = rng.uniform(-0.3, 0.3, CH).astype(np.float32)
    inv = rng.uniform(0.5, 2.0, CH).astype(np.float32)
    wt = (rng.standard_normal((CH, CH, 3, 3)) * 0.1).astype(np.float32)
    # the operand the kernels contract: one fp32 fma, the ReLU, one bf16 rounding
    x = to_bf16(np.maximum(B.z32(y1, bc(sc), bc(sh)), 0.0)).astype(np.float64)
    dw = torch.nn.grad.conv2d_weight(torch.from_numpy(x), (CH, CH, 3, 3), torch.from_numpy(dy), padding=1).numpy()
    return dict(y1=y1, sc=sc, sh=sh, mu=mu, inv=inv, dy=dy, wt=wt, dw=dw)


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_backward_random_operands(env, shape):
    L, E = env
    n, h, w = shape
    r = random_case(shape)
    case = Case(L, E, n, h, w, r["y1"], r["sc"], r["sh"], r["mu"], r["inv"], r["dy"], r["wt"])
    dx, dw, parts = case.launch()
    dx_sep, dw_sep = case.separate()
    assert torch.equal(dx.view(torch.int16), dx_sep.view(torch.int16)), "dX differs from the data-gradient launch"
    # the sums of oct_dact_bn_reduce on dA1 as stored, bound of tests/test_gpu_bn.py::test_dact_bn_reduce
    nhwc = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 2, 3, 1))   # noqa: E731
    ref = B.dact_bn_reduce(nhwc(host(dx)), None, nhwc(r["y1"]), r["sc"], r["sh"], r["mu"], r["inv"])
    tot = parts.astype(np.float64).sum(0)
    reduced(tot[0], ref["s1"], ref["t1"], ref["count"], "bf16", "sum g")
    reduced(tot[1], ref["s2"], ref["t2"], ref["count"] + 3, "bf16", "sum g*xhat")
    # dW: the same fp32 products in another summation order
    e_sep, e_fused = rel_l2(dw_sep, r["dw"]), rel_l2(dw, r["dw"])
    print(f"dW rel L2 error against float64, {shape}: oct_conv_wgrad {e_sep:.3e}, fused {e_fused:.3e}")
    assert e_fused <= 2 * e_sep, (e_fused, e_sep)
    # two launches: identical dX and identical partial rows (dW meets through atomics and is exempt)
    dx2, _, parts2 = case.launch()
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16)), "dX, repeated"
    assert np.array_equal(parts.view(np.int32), parts2.view(np.int32)), "partial rows, repeated (fixed order)"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_descriptors_leave_the_outputs_untouched(env):
    L, E = env
    lib = L.lib()
    n, h, w = 1, 16, 32
    bufs = [torch.full((n * h * w * 64,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    ins = [torch.zeros((n * h * w * 64,), dtype=torch.float32, device="cuda") for _ in range(7)]
    a = L.ConvBwdFusedArgs(*[t.data_ptr() for t in ins], *[t.data_ptr() for t in bufs])
    refused = {
        "f32": desc(L, n, h, w, dt=L.DT_F32), "two sources": desc(L, n, h, w, c1=32), "cout 64": desc(L, n, h, w, cout=64),
        "partials mode": desc(L, n, h, w, partials=1), "cin 64": desc(L, n, h, w, c0=64), "no transform": desc(L, n, h, w, xf=L.XF_NONE),
        "plain affine": desc(L, n, h, w, xf=L.XF_AFFINE), "w % 32": desc(L, 1, 24, 40), "h % 8": desc(L, 1, 12, 32),
    }
    for what, d in refused.items():
        assert lib.oct_conv_backward_fused_ok(C.byref(d)) == 0, what
        assert lib.oct_conv_backward_fused_blocks(C.byref(d)) == 0, what
        assert lib.oct_conv_backward_fused(C.byref(d), C.byref(a), st()) == -22, what
        assert "oct_conv_backward_fused_ok" in L.last_error(), what
    assert lib.oct_conv_backward_fused(None, C.byref(a), st()) == -22
    ok = desc(L, n, h, w)
    assert lib.oct_conv_backward_fused_ok(C.byref(ok)) == 1
    assert lib.oct_conv_backward_fused(C.byref(ok), C.byref(L.ConvBwdFusedArgs()), st()) == -22 and "null tensor" in L.last_error()
    torch.cuda.synchronize()
    for t in bufs:
        assert bool(torch.isnan(t).all()), "a refused launch wrote to its outputs"


def test_engine_keeps_the_separate_launches_where_the_library_refuses(env):
    """(1, 24, 40): W is no multiple of 32.  `_block_backward` asks the library, gets 0, and gives what the separate launches
    give: the same bits as the chain BatchNorm backward -> dW / dX -> reduction -> BatchNorm backward -> dW / dX run by hand
    (weight gradients meet through atomics: to fp32 round-off), and the data gradient of the second convolution agrees with
    float64."""
    L, E = env
    n, h, w = 1, 24, 40
    assert L.lib().oct_conv_backward_fused_ok(C.byref(desc(L, n, h, w))) == 0
    rng = np.random.default_rng(7)
    bf = lambda: to_bf16(rng.standard_normal((n, CH, h, w))).astype(np.float64)   # noqa: E731
    x0, y1, y2, da = bf(), bf(), bf(), bf()
    vec = lambda lo, hi: fdev(rng.uniform(lo, hi, CH))   # noqa: E731
    bn1 = E.BNState(vec(0.5, 1.5), vec(-0.5, 0.5), vec(-0.3, 0.3), vec(0.5, 2.0))
    bn2 = E.BNState(vec(0.5, 1.5), vec(-0.5, 0.5), vec(-0.3, 0.3), vec(0.5, 2.0))
    wt = {k: fdev(rng.standard_normal((CH, CH, 3, 3)) * 0.1) for k in ("w1", "w2")}
    y1d, y2d = dev(y1), dev(y2)
    r1 = E.ConvRec("w1", "g1", "b1", None, E.Src(dev(x0), CH), y1d, bn1, CH, n, h, w)
    r2 = E.ConvRec("w2", "g2", "b2", None, E.Src(y1d, CH, bn1), y2d, bn2, CH, n, h, w)
    eng = E.UNetEngine(1, 2, 4, "bf16")
    eng._P = dict(wt, g1=vec(0.5, 1.5), g2=vec(0.5, 1.5))
    eng._ctx = E.Ctx(n=n, h=h, w=w, convs={"blk": [r1, r2]})

    def grads():
        return {k: torch.full((CH, CH, 3, 3) if k[0] == "w" else (CH,), float("nan"), dtype=torch.float32, device="cuda")
                for k in ("w1", "w2", "g1", "b1", "g2", "b2")}
    asked = []
    orig = eng._conv_backward_fused
    eng._conv_backward_fused = lambda *a, **k: (asked.append(orig(*a, **k)), asked[-1])[1]
    G = grads()
    d0, _ = eng._block_backward("blk", dev(da), None, G, False)
    assert asked == [None], "the engine asks once and is refused"
    # the same chain by hand
    H = grads()
    dy2 = eng._bn_backward(r2, dev(da), None, H, False)
    dy2_host = host(dy2).astype(np.float64)
    da1, _ = eng._conv_backward(r2, dy2, H, False)
    da1_host = host(da1).astype(np.float64)
    dy1 = eng._bn_backward(r1, da1, None, H, False)
    e0, _ = eng._conv_backward(r1, dy1, H, False)
    torch.cuda.synchronize()
    assert torch.equal(d0.view(torch.int16), e0.view(torch.int16)), "dX of the block"
    for k in ("g1", "b1", "g2", "b2"):
        assert torch.equal(G[k], H[k]), k
    for k in ("w1", "w2"):
        assert rel_l2(G[k].cpu().numpy(), H[k].cpu().numpy()) < 1e-5, k
    wq = to_bf16(wt["w2"].cpu().numpy()).astype(np.float64)
    dx, _ = O.conv3x3_bwd(np.zeros((n, CH, h, w)), wq, dy2_host)
    assert rel_l2(da1_host, dx) < 4e-3


# ---- one training step ------------------------------------------------------------------------------------------------------
def test_training_step_with_and_without_the_fused_launches(golden_dir):
    """UNet(1, 8, 32) on the wide fixture's inputs (2 x 64 x 128, the smallest fixture at the headline width): one bf16
    forward_backward with the fused launches (enc1.conv2, dec1.conv2) and one with the separate ones.  The fused launch changes
    no operand, only the order of fp32 sums (dW, the BatchNorm sums) -- whose effect reaches the other gradients through one
    bf16 rounding of dY1.  Yardstick per gradient: the distance of the bf16 step from the fp32 parity-mode step; the two bf16
    steps must be closer than a tenth of it."""
    from oracle.cases import ynet_case
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    z = np.load(os.path.join(golden_dir, "unet_c8_f32_2x64x128_wide.npz"))
    in_ch, ncls, feat, b, h, w = (int(v) for v in z["meta"])
    model, x, t = ynet_case(UNet, int(z["seed"]), in_ch, ncls, feat, (b, h, w))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    x, t = x.cuda(), t.cuda()

    def grads(dtype, fused):
        model.load_state_dict(state)
        model.set_compute_dtype(dtype)
        model._engine.fused_bwd_off = not fused
        calls = []
        if fused:
            orig = model._engine._conv_backward_fused
            model._engine._conv_backward_fused = lambda *a, **k: (calls.append(orig(*a, **k)), calls[-1])[1]
        model.forward_backward(x, t)
        torch.cuda.synchronize()
        if fused:
            del model._engine._conv_backward_fused
            assert sum(c is not None for c in calls) == 2, "enc1.conv2 and dec1.conv2 take the fused launch"
        return {k: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters()}
    g_fused, g_sep, g_f32 = grads("bf16", True), grads("bf16", False), grads("f32", False)
    model._engine.fused_bwd_off = False
    worst = 0.0
    for k in g_sep:
        yard, diff = rel_l2(g_sep[k], g_f32[k]), rel_l2(g_fused[k], g_sep[k])
        print(f"{k}: bf16 vs f32 {yard:.3e}, fused vs separate {diff:.3e}")
        worst = max(worst, diff / yard)
        assert diff < 0.1 * yard, (k, diff, yard)
    print(f"largest fused-vs-separate difference: {worst:.3f} of the bf16-vs-f32 yardstick")
