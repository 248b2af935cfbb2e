"""oct_conv_wgrad with dy_coef + dy_out (wgrad2.hip, DYAPPLY): the weight gradient of dec1.conv1 (two 32-channel sources,
32 output channels) applies the BatchNorm backward of its output when it stages dY and stores dY for the data gradient.

* dy_out is bit for bit what oct_bn_bwd_apply_to writes, into a separate buffer and in place over dA;
* dyadic operands (every fp32 sum exact in any order): dW equals oct_conv_wgrad on the materialised dY bit for bit;
* random operands: dW is no further from float64 than twice the two-launch path's own error (the rule of
  tests/test_gpu_fused_backward.py::test_fused_backward_random_operands);
* descriptors and argument sets the form does not take are refused with the outputs untouched.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C0 = C1 = COUT = 32
# one tile | the contiguous tile walk (8 tiles) | 1536 tiles of 8 x 32: the interleaved walk, three stages per workgroup at
# 512 workgroups, so the two-stage ring of the producers wraps
SHAPES = [(1, 8, 32), (2, 16, 64), (4, 256, 384)]


@pytest.fixture(scope="module")
def env():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    from retinal_oct_image_segmentation_via_deep_learning_amd import engine as E
    L.lib()
    return L, E


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float(torch.sqrt(((a - b) ** 2).sum()) / torch.sqrt((b ** 2).sum()).clamp_min(1e-300))


def desc(L, n, h, w, c0=C0, c1=C1, cout=COUT, partials=0, dt=None):
    return L.WgradDesc(L.DT_BF16 if dt is None else dt, n, h, w, c0, c1, cout, 9, L.XF_NONE, L.XF_AFFINE_RELU if c1 else L.XF_NONE,
                       L.IN_PLAIN, 0, 0, 0, 0, 0, 0, partials)


@functools.lru_cache(maxsize=None)
def operands(shape, exact):
    """NHWC device tensors of one shape, made once and never written: x0 (plain source), x1 + (scale1, shift1) (BN + ReLU
    source), dA, y, coef [3][32], (scale, shift) of the layer's own BatchNorm."""
    n, h, w = shape
    g = torch.Generator().manual_seed(31 * n + 7 * h + w + (1000 if exact else 0))
    npix = n * h * w
    big = npix > 50000      # thin dA, no k1 / k2: the sums of the exact case stay below 2^24 granules (asserted by the test)

    def choice(vals, size):
        return torch.tensor(vals)[torch.randint(0, len(vals), size, generator=g)]
    if exact:
        # integers and dyadic coefficients: x = relu(x1 * s1 + b1) and dY = k0 * mask * dA + k1 * y + k2 are multiples of 1/4 and
        # 1/8 that bf16 holds exactly, and every partial sum of dW stays below 2^24 granules (asserted by the test)
        x0 = torch.randint(-4, 5, (npix, C0), generator=g).float()
        x1 = torch.randint(-4, 5, (npix, C1), generator=g).float()
        s1, b1 = choice([-1.0, -0.5, 0.5, 1.0, 2.0], (C1,)), torch.randint(-2, 3, (C1,), generator=g) * 0.5 + 0.25
        y = torch.randint(-4, 5, (npix, COUT), generator=g).float()
        da = (torch.randint(-2, 3, (npix, COUT), generator=g) * (torch.rand((npix, COUT), generator=g) < (0.04 if big else 0.5))).float()
        sc, sh = choice([-1.0, -0.5, 0.5, 1.0, 2.0], (COUT,)), torch.randint(-2, 3, (COUT,), generator=g) * 0.5 + 0.25
        k0 = choice([-1.0, -0.5, 0.5, 1.0, 2.0], (COUT,))
        k1 = torch.zeros(COUT) if big else choice([-0.25, 0.0, 0.125, 0.25], (COUT,))
        k2 = torch.zeros(COUT) if big else choice([-0.25, 0.0, 0.25, 0.5], (COUT,))
    else:
        x0 = torch.randn((npix, C0), generator=g)
        x1 = torch.randn((npix, C1), generator=g)
        s1 = torch.empty(C1).uniform_(0.5, 1.5, generator=g) * choice([-1.0, 1.0], (C1,))
        b1 = torch.empty(C1).uniform_(-0.5, 0.5, generator=g)
        y = torch.randn((npix, COUT), generator=g)
        da = torch.randn((npix, COUT), generator=g)
        sc = torch.empty(COUT).uniform_(0.5, 1.5, generator=g) * choice([-1.0, 1.0], (COUT,))
        sh = torch.empty(COUT).uniform_(-0.5, 0.5, generator=g)
        # an exact zero of the pre-activation in channel 0: fmaf(0.5, 2, -1)
        sc[0], sh[0] = 2.0, -1.0
        y[torch.rand(npix, generator=g) < 0.2, 0] = 0.5
        k0, k1, k2 = torch.randn(COUT, generator=g), 0.3 * torch.randn(COUT, generator=g), 0.1 * torch.randn(COUT, generator=g)
    act = lambda t, c: t.to(torch.bfloat16).view(n, h, w, c).cuda().contiguous()   # noqa: E731
    f32 = lambda t: t.float().cuda().contiguous()   # noqa: E731
    return dict(x0=act(x0, C0), x1=act(x1, C1), s1=f32(s1), b1=f32(b1), y=act(y, COUT), da=act(da, COUT), sc=f32(sc), sh=f32(sh),
                coef=f32(torch.stack([k0, k1, k2])))


class Runner:
    def __init__(self, L, E, shape, t):
        self.L, self.E, self.shape, self.t = L, E, shape, t
        self.eng = E.UNetEngine(1, 2, 4, "bf16")
        self.src = E.Src(t["x0"], C0, None, t["x1"], C1, E.BNState(t["s1"], t["b1"]))

    def unpack(self, dwp):
        grad = torch.full((COUT, C0 + C1, 3, 3), float("nan"), device="cuda")
        self.eng._unpack(self.L.PACK_CONV_FPROP, dwp, grad, COUT, C0 + C1, False)
        return grad

    def two_launches(self):
        """oct_bn_bwd_apply_to, then oct_conv_wgrad on the dY it wrote -> (dY, dW)"""
        L, t = self.L, self.t
        n, h, w = self.shape
        dy = torch.full((n, h, w, COUT), float("nan"), dtype=torch.bfloat16, device="cuda")
        L.check(L.lib().oct_bn_bwd_apply_to(L.DT_BF16, dy.data_ptr(), t["da"].data_ptr(), t["y"].data_ptr(), t["coef"].data_ptr(),
                                            t["sc"].data_ptr(), t["sh"].data_ptr(), n * h * w, COUT, st()), "oct_bn_bwd_apply_to")
        return dy, self.unpack(self.eng._wgrad(self.src, dy, COUT, 9, n, h, w))

    def fused(self, in_place):
        """one launch -> (dY, dW); in_place: dy_out is the dA tensor (a copy of it: the operands are shared)"""
        t = self.t
        n, h, w = self.shape
        da = t["da"].clone() if in_place else t["da"]
        out = da if in_place else torch.full((n, h, w, COUT), float("nan"), dtype=torch.bfloat16, device="cuda")
        dwp = self.eng._wgrad(self.src, da, COUT, 9, n, h, w, fused_apply=(t["y"], t["coef"], t["sc"], t["sh"]), dy_out=out)
        return out, self.unpack(dwp)


def dw_float64(t, dy, shape):
    """dW[co][ci][ty][tx] = sum dY[p][co] * x[p + (ty - 1, tx - 1)][ci] in float64 on the device, from the operand the kernels
    contract: x = concat(x0, bf16(relu(fmaf(x1, s1, b1))))"""
    n, h, w = shape
    a1 = torch.clamp_min(torch.addcmul(t["b1"], t["x1"].float(), t["s1"]), 0).to(torch.bfloat16)
    x = torch.cat([t["x0"], a1], dim=-1).double()
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    d = dy.double().reshape(-1, COUT)
    out = torch.empty((COUT, C0 + C1, 3, 3), dtype=torch.float64, device="cuda")
    for ty in range(3):
        for tx in range(3):
            out[:, :, ty, tx] = d.T @ xp[:, ty:ty + h, tx:tx + w, :].reshape(-1, C0 + C1)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dy_out_matches_the_apply_launch_and_dw_the_two_launches(env, shape):
    L, E = env
    n, h, w = shape
    assert L.lib().oct_conv_wgrad_apply_store_ok(C.byref(desc(L, n, h, w))) == 1
    t = operands(shape, False)
    run = Runner(L, E, shape, t)
    dy_ref, dw_sep = run.two_launches()
    dy_a, dw_a = run.fused(False)
    dy_b, dw_b = run.fused(True)
    torch.cuda.synchronize()
    z = torch.addcmul(t["sh"].double(), t["y"].double(), t["sc"].double())
    assert int((z[..., 0] == 0).sum()) > 0, "the case holds exact zeros of the pre-activation"
    assert not bool(torch.isnan(dy_a.float()).any()), "a NaN-filled dy_out is overwritten everywhere"
    assert torch.equal(bits(dy_a), bits(dy_ref)), "dy_out (separate buffer) differs from oct_bn_bwd_apply_to"
    assert torch.equal(bits(dy_b), bits(dy_ref)), "dy_out == dy (in place) differs from oct_bn_bwd_apply_to"
    ref = dw_float64(t, dy_ref, shape)
    e_sep, e_a, e_b = rel_l2(dw_sep, ref), rel_l2(dw_a, ref), rel_l2(dw_b, ref)
    print(f"dW rel L2 error against float64, {shape}: two launches {e_sep:.3e}, fused {e_a:.3e}, fused in place {e_b:.3e}")
    assert e_a <= 2 * e_sep and e_b <= 2 * e_sep, (e_a, e_b, e_sep)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_operands_give_the_same_dw_bits(env, shape):
    L, E = env
    t = operands(shape, True)
    run = Runner(L, E, shape, t)
    dy_ref, dw_sep = run.two_launches()
    dy_b, dw_b = run.fused(True)
    torch.cuda.synchronize()
    # the premise: dY and x are held exactly, and the largest sum of |terms| of one dW element is below 2^24 granules (1/32)
    k = t["coef"].double()
    z = torch.addcmul(t["sh"].double(), t["y"].double(), t["sc"].double())
    assert bool((z != 0).all())
    dy64 = k[0] * torch.where(z > 0, t["da"].double(), torch.zeros((), dtype=torch.float64, device="cuda")) + k[1] * t["y"].double() + k[2]
    assert torch.equal(dy64, dy_ref.double()), "dY is exact"
    xmax = 16.0
    assert float(dy64.abs().sum(dim=(0, 1, 2)).max()) * xmax * 32 < 2 ** 24
    assert torch.equal(bits(dy_b), bits(dy_ref))
    assert torch.equal(dw_b.view(torch.int32), dw_sep.view(torch.int32)), "dW differs from oct_conv_wgrad on the materialised dY"
    assert torch.equal(dw_b.double(), dw_float64(t, dy_ref, shape)), "dW is the exact sum"


def test_refusals_leave_the_outputs_untouched(env):
    L, E = env
    lib = L.lib()
    cases = {
        "multi-column grid (128 -> 128)": desc(L, 1, 16, 32, c0=128, c1=0, cout=128),
        "64 -> 64": desc(L, 1, 16, 32, c0=32, c1=32, cout=64),
        "ragged width": desc(L, 1, 16, 40),
        "ragged height": desc(L, 1, 12, 32),
        "partials mode": desc(L, 1, 16, 32, partials=1),
        "f32": desc(L, 1, 16, 32, dt=L.DT_F32),
    }
    big = 16 * 40 * 128
    ins = [torch.zeros(big, dtype=torch.float32, device="cuda") for _ in range(10)]
    dwp = torch.full((4 * 9 * 128 * 128,), float("nan"), device="cuda")
    out = torch.full((big,), float("nan"), device="cuda")
    p = [t.data_ptr() for t in ins]

    def args(dy_out):
        return L.WgradArgs(p[0], p[1], p[2], p[3], p[4], p[5], p[6], dwp.data_ptr(), None, p[7], p[8], p[9], p[9], None, dy_out)
    for what, d in cases.items():
        assert lib.oct_conv_wgrad_apply_store_ok(C.byref(d)) == 0, what
        assert lib.oct_conv_wgrad(C.byref(d), C.byref(args(out.data_ptr())), st()) == -22, what
        assert "oct_conv_wgrad_apply_store_ok" in L.last_error(), what
    ok = desc(L, 1, 16, 32)
    assert lib.oct_conv_wgrad_apply_store_ok(C.byref(ok)) == 1
    assert lib.oct_conv_wgrad_apply_store_ok(None) == 0
    # dy_coef without dy_out keeps the refusal off the first-layer path; dy_out without dy_coef is refused too
    assert lib.oct_conv_wgrad(C.byref(ok), C.byref(args(None)), st()) == -22 and "first layer" in L.last_error()
    a = args(out.data_ptr())
    a.dy_coef = None
    assert lib.oct_conv_wgrad(C.byref(ok), C.byref(a), st()) == -22 and "dy_out" in L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dwp).all()) and bool(torch.isnan(out).all()), "a refused launch wrote to its outputs"
