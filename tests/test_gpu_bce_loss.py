"""GPU: the binary / multi-label loss head (sigmoid BCE + soft Dice, the oct_bce_loss_* kernels of csrc/seg_loss.hip) against
the float64 restatement tests/bce_ref.py (pinned to torch autograd by tests/test_bce_loss_cpu.py), the functional
binary_cross_entropy_dice against torch on the device, and forward_backward_binary / loss_binary / predict_mask of the
networks against torch's BCE through autograd.

Tolerances are the CE kernels' for the same arithmetic (fp32 per element, fp64 sums): loss rtol 1e-5 / atol 1e-7, gradient
1e-5 of its maximum in fp32, one bf16 ulp of the reference (or 1e-6 of the maximum) element-wise in bf16."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bce_ref as R
from test_gpu_seg_loss import LOOSE, _bf16_ulp, _close, _sd_net

pytestmark = pytest.mark.gpu

LAYOUTS = ["nhwc_bf16", "nhwc_f32", "nchw_f32"]
SMALL = (3, 37, 53)      # 5,883 pixels: 22 full tiles of 256 and a 251-pixel tail
LARGE = (2, 360, 368)    # 264,960 pixels = 1,035 tiles > SEG_MAX_GRID = 1,024: the grid-stride loop runs
IGNORE = 255


def _L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    return _lib


@functools.lru_cache(maxsize=8)
def _case(shape, classes, bf16, options):
    """NCHW float64 logits (bf16-representable for the bf16 layout), uint8 masks, and with `options` pos_weight, a map and
    ignore_value 255 on about 20 % of the elements"""
    n, h, w = shape
    g = torch.Generator().manual_seed(classes * 1000 + h + (7 if options else 0))
    x = 3.0 * torch.randn(n, classes, h, w, generator=g)
    if bf16:
        x = x.to(torch.bfloat16).float()
    t = (torch.rand(n, classes, h, w, generator=g) < 0.35).to(torch.uint8)
    kw = {}
    if options:
        t[torch.rand(n, classes, h, w, generator=g) < 0.2] = IGNORE
        kw = dict(pos_weight=(0.25 + 3.75 * torch.rand(classes, generator=g)).numpy(),
                  pixel_weight=(1.0 + 9.0 * (torch.rand(n, h, w, generator=g) < 0.1).float()).numpy(), ignore_value=IGNORE)
    return x.double().numpy(), t.numpy(), kw


@functools.lru_cache(maxsize=8)
def _reference(shape, classes, bf16, options, w_dice):
    x, t, kw = _case(shape, classes, bf16, options)
    return R.loss_and_grad(x, t, 1.0, w_dice, **kw)


def _device_logits(layout, x, offset=0):
    """the logits in `layout` on the device; offset: the view starts that many elements into its storage"""
    xt = torch.from_numpy(x).float()
    if layout != "nchw_f32":
        xt = xt.permute(0, 2, 3, 1).contiguous()
    if layout == "nhwc_bf16":
        xt = xt.to(torch.bfloat16)
    if not offset:
        return xt.cuda()
    buf = torch.empty(xt.numel() + offset, dtype=xt.dtype, device="cuda")
    view = buf[offset:].view(xt.shape)
    view.copy_(xt)
    return view


def _nan_like(lg, offset=0):
    buf = torch.full((lg.numel() + offset,), float("nan"), dtype=lg.dtype, device="cuda")
    return buf[offset:].view(lg.shape)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().cuda()


class Plan:
    """the three entry points through the C ABI for one logits tensor, every output pre-filled with NaN"""

    def __init__(self, layout, lg, t, kw):
        L = self.L = _L()
        self.lib = L.lib()
        self.layout, self.lg, self.t = layout, lg, t
        self.n, self.c, self.h, self.w = t.shape
        self.lay = L.SEG_NCHW if layout == "nchw_f32" else L.SEG_NHWC
        self.d = L.HeadDesc(L.DT_BF16 if lg.dtype == torch.bfloat16 else L.DT_F32, self.n, self.h, self.w, 1, self.c)
        self.nb = self.lib.oct_seg_loss_blocks(self.n * self.h * self.w, self.c)
        self.pos, self.pm = _dev(kw.get("pos_weight")), _dev(kw.get("pixel_weight"))
        self.has = int(kw.get("ignore_value") is not None)
        self.ig = kw.get("ignore_value") or 0
        self.needs_wsum = self.pm is not None or self.has
        self.st = torch.cuda.current_stream().cuda_stream

    def rows(self):
        return torch.full((self.nb, self.L.HEAD_LOSS_SLOTS), float("nan"), dtype=torch.float64, device="cuda")

    def forward(self, want_dice, tau=0.0, mask=None, rows=True, target=True):
        part = self.rows() if rows else None
        self.L.check(self.lib.oct_bce_loss_forward(C.byref(self.d), self.lay, self.lg.data_ptr(), self.t.data_ptr() if target else None,
                                                   self.L.ptr(self.pos), self.L.ptr(self.pm), self.has, self.ig, int(want_dice),
                                                   float(tau), self.L.ptr(mask), self.L.ptr(part), self.st))
        return part

    def finalize(self, part, w_dice):
        out = torch.full((3,), float("nan"), device="cuda")
        coef = torch.full((2 * self.L.MAX_CLASSES,), float("nan"), device="cuda")
        wsum = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        self.L.check(self.lib.oct_seg_loss_finalize_weighted(C.byref(self.d), part.data_ptr(), self.nb, 1.0, w_dice, 1e-7,
                                                             out.data_ptr(), coef.data_ptr(), wsum.data_ptr(), self.st))
        return out, coef, wsum

    def weight_sum(self):
        scratch = torch.full((self.nb + 1,), float("nan"), dtype=torch.float64, device="cuda")
        self.L.check(self.lib.oct_bce_loss_weight_sum(C.byref(self.d), self.t.data_ptr(), self.L.ptr(self.pm), self.has, self.ig,
                                                      scratch.data_ptr(), scratch[self.nb:].data_ptr(), self.st))
        return scratch[self.nb:]

    def backward(self, wsum, coef, dloss=None, part=None, offset=0):
        dl = _nan_like(self.lg, offset)
        self.L.check(self.lib.oct_bce_loss_backward(C.byref(self.d), self.lay, self.lg.data_ptr(), self.t.data_ptr(),
                                                    self.L.ptr(self.pos), self.L.ptr(self.pm), self.has, self.ig, self.L.ptr(wsum),
                                                    self.L.ptr(coef), 1.0, self.L.ptr(dloss), dl.data_ptr(), self.L.ptr(part), self.st))
        return dl

    def nchw(self, dl):
        d = dl.float() if self.layout == "nchw_f32" else dl.float().permute(0, 3, 1, 2)
        return d.cpu().double().numpy()


def _run(layout, lg, t, kw, w_dice, dloss=None, offset=0, nan_loss=False):
    """forward -> finalize -> backward, and for w_dice == 0 the one-pass schedule as well (weight_sum -> backward with rows ->
    finalize), which must give the same bits: ([loss, bce, dice], dlogits NCHW float64, rows, raw dlogits)"""
    p = Plan(layout, lg, t, kw)
    part = p.forward(w_dice != 0.0)
    assert nan_loss or not torch.isnan(part).any()         # every row was written
    out, coef, wsum = p.finalize(part, w_dice)
    dl = p.backward(wsum if p.needs_wsum else None, coef if w_dice else None, dloss, offset=offset)
    if w_dice == 0.0:
        rows = p.rows()
        dl2 = p.backward(p.weight_sum() if p.needs_wsum else None, None, dloss, part=rows, offset=offset)
        assert nan_loss or not torch.isnan(rows).any()
        out2 = p.finalize(rows, 0.0)[0]
        if nan_loss:
            assert bool(torch.isnan(out2[:2]).all()) and bool(torch.isnan(out[:2]).all())
        else:
            assert torch.equal(_bits(out2[:2]), _bits(out[:2])), (out2, out)    # the backward's rows finalise to the forward's bits
            assert torch.equal(_bits(dl2), _bits(dl))                           # and sum omega has the same bits on both routes
        assert float(out[2]) == 0.0
    return out.cpu().numpy(), p.nchw(dl), part, dl


def _check(layout, got, dl, ref, rdl):
    print(f"loss {got} ref {ref}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-7)
    scale = float(np.abs(rdl).max())
    err = np.abs(dl - rdl)
    print(f"gradient: max err {np.nanmax(err):.3e}, scale {scale:.3e}")
    assert not np.isnan(dl).any()            # every element was written
    if layout == "nhwc_bf16":
        assert (err <= np.maximum(_bf16_ulp(rdl), 1e-6 * scale)).all(), float((err / _bf16_ulp(rdl)).max())
    else:
        assert err.max() <= 1e-5 * scale, (err.max(), scale)


def _bits(a):
    return a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32 if a.dtype == torch.float32 else torch.int64)


def _kernels_case(layout, classes, w_dice, options, shape, offset=0):
    bf16 = layout == "nhwc_bf16"
    x, t, kw = _case(shape, classes, bf16, options)
    ref, rdl = _reference(shape, classes, bf16, options, w_dice)
    lg, td = _device_logits(layout, x, offset), torch.from_numpy(t).cuda()
    got, dl, part, raw = _run(layout, lg, td, kw, w_dice, offset=offset)
    _check(layout, got, dl, ref, rdl)
    if options:
        assert (dl[t == IGNORE] == 0).all()
    # deterministic: a second run gives the same bits
    got2, _, part2, raw2 = _run(layout, lg, td, kw, w_dice, offset=offset)
    assert np.array_equal(got, got2) and torch.equal(_bits(raw), _bits(raw2)) and torch.equal(_bits(part), _bits(part2))


# ---- 1. the kernels against bce_ref through the C ABI --------------------------------------------------------------------
@pytest.mark.parametrize("options", [False, True])
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
@pytest.mark.parametrize("classes", [1, 3, 8, 11, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernels_match_the_float64_reference(layout, classes, w_dice, options):
    _kernels_case(layout, classes, w_dice, options, SMALL)


@pytest.mark.parametrize("options", [False, True])
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
@pytest.mark.parametrize("classes", [1, 3])
def test_kernels_match_the_reference_past_the_grid_limit(classes, w_dice, options):
    assert _L().lib().oct_seg_loss_blocks(LARGE[0] * LARGE[1] * LARGE[2], classes) == 1024
    _kernels_case("nhwc_bf16", classes, w_dice, options, LARGE)


@pytest.mark.parametrize("options", [False, True])
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
def test_kernels_match_the_reference_on_views_that_are_not_16_byte_aligned(w_dice, options):
    _kernels_case("nhwc_bf16", 3, w_dice, options, SMALL, offset=1)


# ---- 2. ignored elements and bad labels ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ignored_elements_and_bad_labels(layout, w_dice):
    bf16 = layout == "nhwc_bf16"
    x, t, kw = _case(SMALL, 3, bf16, True)
    td = torch.from_numpy(t).cuda()
    base, bdl, _, _ = _run(layout, _device_logits(layout, x), td, kw, w_dice)
    ign = t == IGNORE
    assert ign.any() and (bdl[ign] == 0).all()
    for bad in (np.nan, np.inf, -np.inf):         # a logit under an ignored element cannot leak
        x2 = np.where(ign, bad, x)
        got, dl, _, _ = _run(layout, _device_logits(layout, x2), td, kw, w_dice)
        assert np.array_equal(got, base), (bad, got, base)
        assert (dl[ign] == 0).all() and np.array_equal(dl, bdl)
    # everything ignored: NaN; a valid label of 7: NaN
    lg = _device_logits(layout, x)
    assert np.isnan(_run(layout, lg, torch.full_like(td, IGNORE), kw, w_dice, nan_loss=True)[0][0])
    t7 = td.clone()
    t7[tuple(int(v) for v in np.argwhere(~ign)[0])] = 7
    assert np.isnan(_run(layout, lg, t7, kw, w_dice, nan_loss=True)[0][0])
    assert np.isnan(_run(layout, lg, t7.clamp(0, 7), {}, w_dice, nan_loss=True)[0][0])
    # identity options: the no-option result within the bounds of test 1
    x0, t0, _ = _case(SMALL, 3, bf16, False)
    ref, rdl = _reference(SMALL, 3, bf16, False, w_dice)
    ident = dict(pos_weight=np.ones(3, np.float32), pixel_weight=np.ones(SMALL, np.float32), ignore_value=200)
    got, dl, _, _ = _run(layout, _device_logits(layout, x0), torch.from_numpy(t0).cuda(), ident, w_dice)
    _check(layout, got, dl, ref, rdl)


# ---- 3. the upstream gradient -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_upstream_gradient_scales_dlogits(layout, options):
    x, t, kw = _case(SMALL, 3, layout == "nhwc_bf16", options)
    lg, td = _device_logits(layout, x), torch.from_numpy(t).cuda()
    for w_dice in (0.0, 0.7):
        _, dl1, _, _ = _run(layout, lg, td, kw, w_dice)
        _, dlg, _, _ = _run(layout, lg, td, kw, w_dice, dloss=torch.tensor([0.25], device="cuda"))
        np.testing.assert_allclose(dlg, 0.25 * dl1, rtol=1e-6 if layout != "nhwc_bf16" else 1e-2, atol=0)


# ---- 4. the mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.5, 0.3])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mask_is_logits_at_or_above_tau(layout, threshold):
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import mask_threshold
    tau = mask_threshold(threshold)
    assert tau == R.threshold_to_tau(threshold)
    x, t, kw = _case(SMALL, 3, layout == "nhwc_bf16", False)
    x = x.copy()
    x[0, 1, 5, 6] = x[2, 2, 36, 52] = tau          # equal to tau gives 1 (in bf16: whatever tau rounds to, by the same rule)
    x[1, 0, 7, 8] = np.nan                         # NaN gives 0
    lg = _device_logits(layout, x)
    stored = (lg.float() if layout == "nchw_f32" else lg.float().permute(0, 3, 1, 2)).cpu().numpy()
    want = R.mask(stored, tau)
    assert want[1, 0, 7, 8] == 0 and (layout == "nhwc_bf16" and threshold != 0.5 or want[0, 1, 5, 6] == 1)
    p = Plan(layout, lg, torch.from_numpy(t).cuda(), kw)
    mask = torch.full(t.shape, 9, dtype=torch.uint8, device="cuda")
    p.forward(False, tau=tau, mask=mask, rows=False, target=False)       # no target: the mask alone, no rows
    assert np.array_equal(mask.cpu().numpy(), want)
    assert 0 < int(mask.sum()) < mask.numel()
    # with the loss rows in the same launch: the same mask, and the rows of a launch without one
    mask2 = torch.full_like(mask, 9)
    rows = p.forward(True, tau=tau, mask=mask2)
    assert torch.equal(mask2, mask) and torch.equal(_bits(rows), _bits(p.forward(True)))


# ---- 5. the functional loss against torch on the device -----------------------------------------------------------------
def _torch_binary(out, t, w_bce=1.0, w_dice=0.0, pos=None, pm=None, ig=None, eps=1e-7):
    """torch's loss on the device: (omega * BCEWithLogits(pos_weight=, reduction='none')).sum() / omega.sum() + a torch Dice"""
    t = t.reshape(out.shape)
    c = out.shape[1]
    valid = torch.ones_like(t, dtype=torch.bool) if ig is None else t != ig
    tf = torch.where(valid, t, torch.zeros_like(t)).float()
    per = F.binary_cross_entropy_with_logits(out, tf, pos_weight=None if pos is None else pos.view(1, c, 1, 1), reduction="none")
    omega = valid.float() * (1.0 if pm is None else pm[:, None])
    loss = w_bce * (omega * per).sum() / omega.sum()
    if w_dice:
        s, v = torch.sigmoid(out), valid.float()
        inter, ps, ys = (s * tf * v).sum((0, 2, 3)), (s * v).sum((0, 2, 3)), (tf * v).sum((0, 2, 3))
        loss = loss + w_dice * (1.0 - ((2.0 * inter + eps) / (ps + ys + eps)).mean())
    return loss


@pytest.mark.parametrize("classes", [1, 3])
def test_binary_cross_entropy_dice_is_torch_bce_and_differentiates(classes):
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import binary_cross_entropy_dice
    x, t, _ = _case(SMALL, classes, False, False)
    td = torch.from_numpy(t).cuda()
    if classes == 1:
        td = td[:, 0].contiguous()                      # (B, H, W) for one channel
    a = torch.from_numpy(x).float().cuda().requires_grad_(True)
    b = a.detach().clone().requires_grad_(True)
    la = binary_cross_entropy_dice(a, td)
    lb = F.binary_cross_entropy_with_logits(b, td.reshape(b.shape).float())
    assert la.dim() == 0 and la.requires_grad
    (2.0 * la).backward()
    (2.0 * lb).backward()
    np.testing.assert_allclose(float(la.detach()), float(lb.detach()), rtol=2e-5)
    assert float((a.grad - b.grad).abs().max()) <= 2e-3 * float(b.grad.abs().max())
    # a bool target is the same mask
    assert torch.equal(binary_cross_entropy_dice(a.detach(), td.bool()), la.detach())
    # all three options and a Dice term
    xo, to, kw = _case(SMALL, classes, False, True)
    tod, pos, pm = torch.from_numpy(to).cuda(), _dev(kw["pos_weight"]), _dev(kw["pixel_weight"])
    c = torch.from_numpy(xo).float().cuda().requires_grad_(True)
    e = c.detach().clone().requires_grad_(True)
    lc = binary_cross_entropy_dice(c, tod, 0.8, 0.7, pos_weight=[float(v) for v in kw["pos_weight"]], pixel_weight=pm,
                                   ignore_value=IGNORE)
    le = _torch_binary(e, tod, 0.8, 0.7, pos, pm, IGNORE)
    lc.backward()
    le.backward()
    np.testing.assert_allclose(float(lc.detach()), float(le.detach()), rtol=2e-5)
    assert float((c.grad - e.grad).abs().max()) <= 2e-3 * float(e.grad.abs().max())
    assert (c.grad[tod == IGNORE] == 0).all()


# ---- 6. the networks, fp32 ----------------------------------------------------------------------------------------------
ZERO_UP_TO_ROUNDING = 1e-6      # test_gpu_seg_loss_weighted.py: both sides below it, vectors only

NETS = {"AttU_Net": (1, (2, 32, 48)), "U_Net": (1, (1, 32, 32)), "MGUNet_2": (2, (2, 48, 64)), "ReLayNet": (2, (2, 32, 48)),
        "BioUNet": (1, (2, 16, 24)), "UNet": (1, (2, 32, 32))}


def _ctor(name):
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.BioNet_2020 import UNet as BioUNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net import unet as U
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.ReLayNet_2017 import ReLayNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.YNet_2022 import UNet
    return {"AttU_Net": lambda ci, nc: U.AttU_Net(ci, nc, channels=[4, 8, 16, 32, 64], compute_dtype="f32"),
            "U_Net": lambda ci, nc: U.U_Net(ci, nc, compute_dtype="f32"),
            "MGUNet_2": lambda ci, nc: M.MGUNet_2(ci, nc, feature_scale=16, compute_dtype="f32"),
            "ReLayNet": lambda ci, nc: ReLayNet(ci, nc, num_filters=8, compute_dtype="f32"),
            "BioUNet": lambda ci, nc: BioUNet(ci, nc, compute_dtype="f32"),
            "UNet": lambda ci, nc: UNet(ci, nc, init_features=4, compute_dtype="f32")}[name]


def _binary_options_for(n, c, h, w, seed):
    """(uint8 masks with about 20 % of the elements ignored, pos_weight, map) on the device; masks may overlap"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(n, c, h, w, generator=g) < 0.4).to(torch.uint8)
    t[torch.rand(n, c, h, w, generator=g) < 0.2] = IGNORE
    pos = 0.25 + 3.75 * torch.rand(c, generator=g)
    pm = 1.0 + 9.0 * (torch.rand(n, h, w, generator=g) < 0.1).float()
    return t.cuda(), pos.cuda(), pm.cuda()


@pytest.mark.parametrize("name", list(NETS))
def test_f32_forward_backward_binary_matches_torch_bce_through_autograd(name):
    from oracle.cases import bio_case
    ncls, (n, h, w) = NETS[name]
    a, x, _ = bio_case(_ctor(name), 41, n, 1, ncls, h, w)
    b = bio_case(_ctor(name), 41, n, 1, ncls, h, w)[0]
    a, b, xd = a.cuda().train(), b.cuda().train(), x.cuda()
    td, pos, pm = _binary_options_for(n, ncls, h, w, 42)
    if ncls == 2:
        assert int(((td[:, 0] == 1) & (td[:, 1] == 1)).sum()) > 0          # the two masks overlap
    out = a.forward_backward_binary(xd, td, pos_weight=pos, pixel_weight=pm, ignore_value=IGNORE)
    assert out.shape == (3,) and out.device.type == "cuda"
    if name == "UNet":
        # forward() returns the softmax (1 everywhere for one channel): torch's loss on the logits, the engine's backward
        P = b._tensors()
        ectx, _, _, lg = b._engine.forward(P, xd, train=True, want_probs=False, want_logits=True)
        leaf = lg.detach().clone().requires_grad_(True)
        ref = _torch_binary(leaf, td, 1.0, 0.0, pos, pm, IGNORE)
        ref.backward()
        G = {}
        for k, p in b.named_parameters():
            p.grad = torch.empty_like(p.data)
            G[k] = p.grad
        b._engine.backward(P, ectx, G, dlogits=leaf.grad)
    else:
        ref = _torch_binary(b(xd), td, 1.0, 0.0, pos, pm, IGNORE)
        ref.backward()
    loss = out.cpu().numpy()
    print(f"loss {loss[0]:.8f} torch {float(ref):.8f}")
    np.testing.assert_allclose(loss[0], float(ref.detach()), rtol=2e-5)
    np.testing.assert_allclose(loss[1], loss[0], rtol=0)
    assert loss[2] == 0.0
    gb = dict(b.named_parameters())
    compared = 0
    for k, p in a.named_parameters():
        ga, gr = p.grad.cpu().numpy(), gb[k].grad.cpu().numpy()
        if max(float(np.abs(ga).max()), float(np.abs(gr).max())) <= ZERO_UP_TO_ROUNDING:
            print(f"{k}: zero up to rounding on both sides ({np.abs(ga).max():.3e}, {np.abs(gr).max():.3e})")
            assert ga.ndim == 1, k            # biases and BatchNorm vectors only: every weight tensor is compared
            continue
        _close(ga, gr, k, 2e-3)
        compared += 1
    assert compared > len(gb) // 2
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        if "running" in k:
            _close(sa[k].cpu().numpy(), sb[k].cpu().numpy(), k, 1e-4)
    nbt = [k for k in sa if k.endswith("num_batches_tracked")]
    assert nbt and all(int(sa[k]) == 1 for k in nbt)


# ---- 7. fused equals functional -----------------------------------------------------------------------------------------
WIDE = dict(channels=[16, 32, 64, 128, 256])


@pytest.mark.parametrize("w_dice", [0.0, 0.5])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_backward_binary_equals_the_functional_path(dtype, w_dice):
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import binary_cross_entropy_dice
    m = _sd_net("AttU_Net", dtype, WIDE, classes=1)
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(5)).cuda()
    td, pos, pm = _binary_options_for(2, 1, 32, 48, 32)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    e = ops.kernels(dtype)
    keep = e.deterministic
    try:
        e.deterministic = True
        for kw in ({}, dict(pos_weight=pos, pixel_weight=pm, ignore_value=IGNORE)):
            tk = td if kw else td.clamp(0, 1)
            m.load_state_dict(init)
            m.zero_grad(set_to_none=True)
            loss = binary_cross_entropy_dice(m(x), tk, 1.0, w_dice, **kw)
            loss.backward()
            a, la = {k: p.grad.clone() for k, p in m.named_parameters()}, float(loss.detach())
            m.load_state_dict(init)
            out = m.forward_backward_binary(x, tk, 1.0, w_dice, **kw)
            b = {k: p.grad.clone() for k, p in m.named_parameters()}
            bad = [k for k in a if not (torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-7) if k in LOOSE else torch.equal(a[k], b[k]))]
            assert bad == [], bad
            assert la == float(out[0])
            assert float(out[2]) > 0.0 if w_dice else float(out[2]) == 0.0
    finally:
        e.deterministic = keep


# ---- 8. contracts --------------------------------------------------------------------------------------------------------
def _small_unet(seed=50):
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    torch.manual_seed(seed)
    return UNet(1, 1, init_features=8, compute_dtype="f32").cuda().train()


@pytest.mark.parametrize("net", ["UNet", "AttU_Net"])
def test_forward_backward_binary_contracts(net):
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import mask_threshold
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    engine = net == "UNet"
    m = _small_unet() if engine else _sd_net("AttU_Net", "f32", WIDE, classes=1)
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(6)).cuda()
    td, pos, pm = _binary_options_for(2, 1, 32, 48, 6)
    kw = dict(pos_weight=pos, pixel_weight=pm, ignore_value=IGNORE)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    e = ops.kernels("f32")
    keep = e.deterministic
    try:
        e.deterministic = True
        for w_dice in (0.0, 0.5):
            m.load_state_dict(init)
            l1 = m.forward_backward_binary(x, td[:, 0], 1.0, w_dice, **kw)            # (B, H, W) for one channel
            sd = m.state_dict()
            nbt = [k for k in sd if k.endswith("num_batches_tracked")]
            assert nbt and all(int(sd[k]) == 1 for k in nbt)                 # one forward's worth
            ids = {k: id(p.grad) for k, p in m.named_parameters()}
            m.load_state_dict(init)
            m.forward_backward_binary(x, td, 1.0, w_dice, **kw)
            for k, p in m.named_parameters():
                assert id(p.grad) == ids[k]                                   # overwritten in place, same tensors
            # loss_binary() in train mode: the loss forward_backward_binary returned
            m.load_state_dict(init)
            l3 = m.loss_binary(x, td, 1.0, w_dice, **kw)
            if w_dice:
                assert torch.equal(l3, l1) and float(l1[2]) > 0.0
            else:
                assert torch.equal(l3[:2], l1[:2]) and float(l1[2]) == 0.0   # a BCE-only step does not accumulate the Dice sums
    finally:
        e.deterministic = keep
    # FusedSGD keeps the flat views: the binary step writes into them
    m.load_state_dict(init)
    opt = FusedSGD(list(m.named_parameters()), lr=0.01, momentum=0.9)
    for _ in range(2):
        m.forward_backward_binary(x, td, **kw)
        opt.step()
    for (k, p), o in zip(m.named_parameters(), opt.layout.offsets):
        assert p.grad.data_ptr() == opt.flat_g[o:].data_ptr(), k
    assert float(opt.flat_g.abs().sum()) > 0 and bool(torch.isfinite(opt.flat_g).all())
    # predict_mask == logits >= tau, exactly, in both modes
    for mode in (True, False):
        for thr in (0.5, 0.3):
            m.train(mode)
            with torch.no_grad():
                want = (m.logits(x) if engine else m(x)) >= mask_threshold(thr)
            got = m.predict_mask(x, thr)
            assert got.dtype == torch.uint8 and got.shape == (2, 1, 32, 48) and torch.equal(got.bool(), want)
    with pytest.raises(RuntimeError, match="needs train"):
        m.eval().forward_backward_binary(x, td, **kw)


def test_unet_stage_hook_sees_every_stage_on_the_binary_route():
    m = _small_unet()
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(9)).cuda()
    td, pos, pm = _binary_options_for(2, 1, 32, 48, 9)

    class Hook:
        flush_stages = set(range(len(m._engine.backward_stages())))

        def __init__(self):
            self.seen = []

        def stage_done(self, idx):
            self.seen.append(idx)

    hook = Hook()
    out = m.forward_backward_binary(x, td, 1.0, 0.5, stage_hook=hook, pos_weight=pos, pixel_weight=pm, ignore_value=IGNORE)
    assert hook.seen == sorted(Hook.flush_stages)
    assert bool(torch.isfinite(out).all())


# ---- 9. it trains --------------------------------------------------------------------------------------------------------
def test_ten_steps_lower_the_loss_and_the_masks_feed_the_metrics():
    from retinal_oct_image_segmentation_via_deep_learning_amd.Metrics.Region_based_metrics import dice_coefficient
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    m = _sd_net("AttU_Net", "f32", dict(channels=[4, 8, 16, 32, 64]), classes=1, seed=13)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(2, 1, 32, 48, generator=g).cuda()
    mask = (x > 0.3).to(torch.uint8)                       # something a network can learn from the pixel itself
    opt = FusedSGD(list(m.named_parameters()), lr=0.02, momentum=0.9)
    losses = []
    for _ in range(10):
        losses.append(m.forward_backward_binary(x, mask, 1.0, 0.5))
        opt.step()
    losses = torch.stack(losses).cpu().numpy()
    print("losses", losses[:, 0])
    assert np.isfinite(losses).all() and losses[-1, 0] < losses[0, 0]
    pred = m.predict_mask(x)
    got = float(dice_coefficient(mask, pred))
    tn, pn = mask.cpu().numpy().astype(np.float64), pred.cpu().numpy().astype(np.float64)
    want = 2.0 * (tn * pn).sum() / (tn.sum() + pn.sum() + 1e-7)
    np.testing.assert_allclose(got, want, rtol=1e-12)


# ---- 10. the trainer -----------------------------------------------------------------------------------------------------
def test_data_parallel_trainer_runs_the_binary_loss():
    """world size 1, deterministic, the atomics-summed biases (LOOSE) frozen: two binary trainer steps == by hand, to the bit"""
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp, ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(7)).cuda()
    td, pos, pm = _binary_options_for(2, 1, 32, 48, 7)
    e = ops.kernels("f32")
    keep = e.deterministic
    res = []
    try:
        e.deterministic = True
        for by_hand in (False, True):
            m = _sd_net("AttU_Net", "f32", WIDE, classes=1, seed=12)
            for k, p in m.named_parameters():
                p.requires_grad_(k not in LOOSE)
            if by_hand:
                opt = FusedSGD(list(m.named_parameters()), lr=0.01, momentum=0.9)
                for _ in range(2):
                    m.forward_backward_binary(x, td, 1.0, 0.3, pos_weight=pos, pixel_weight=pm, ignore_value=IGNORE)
                    opt.step()
            else:
                tr = ddp.DataParallelTrainer(m, lr=0.01, momentum=0.9, w_dice=0.3, loss="binary", pos_weight=pos.tolist(),
                                             ignore_value=IGNORE)
                assert torch.equal(tr.pos_weight, pos)       # the sequence was converted once
                for _ in range(2):
                    loss = tr.step(x, td, pixel_weight=pm)
                assert bool(torch.isfinite(loss).all())
            res.append({k: p.detach().clone() for k, p in m.named_parameters()})
    finally:
        e.deterministic = keep
    bad = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
    assert bad == [], bad
    moved = _sd_net("AttU_Net", "f32", WIDE, classes=1, seed=12)
    assert not torch.equal(moved.Conv1.init_conv.weight.cuda(), res[0]["Conv1.init_conv.weight"])
