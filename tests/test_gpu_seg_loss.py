"""GPU: the CE + soft-Dice loss kernels on network logits (csrc/seg_loss.hip) against the float64 oracle
(oracle/ref_cpu.py::loss_head_fwd / loss_head_bwd), the functional cross_entropy_dice, and the forward_backward / loss /
predict extras of the logits networks against the reference fixtures and the torch-CE path."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from oracle.cases import bio_case, bio_grad_errors, bio_weights_match

pytestmark = pytest.mark.gpu

LAYOUTS = ["nhwc_bf16", "nhwc_f32", "nchw_f32"]


def _L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    return _lib


@functools.lru_cache(maxsize=4)
def _logits(shape, classes, bf16):
    """NCHW float64 logits (bf16-representable for the bf16 layout) and labels, seeded by the case"""
    n, h, w = shape
    g = torch.Generator().manual_seed(classes * 1000 + h)
    x = 3.0 * torch.randn(n, classes, h, w, generator=g)
    if bf16:
        x = x.to(torch.bfloat16).float()
    t = torch.randint(0, classes, (n, h, w), generator=g)
    return x.double().numpy(), t.numpy()


@functools.lru_cache(maxsize=4)
def _oracle(shape, classes, bf16, w_dice):
    x, t = _logits(shape, classes, bf16)
    loss, ce, dice, cache = ref_cpu.loss_head_fwd(x, t, 1.0, w_dice)
    return np.array([loss, ce, dice]), ref_cpu.loss_head_bwd(cache, 1.0, w_dice)


def _device_logits(layout, x):
    xt = torch.from_numpy(x).float().cuda()
    if layout == "nchw_f32":
        return xt.contiguous()
    xt = xt.permute(0, 2, 3, 1).contiguous()
    return xt.to(torch.bfloat16) if layout == "nhwc_bf16" else xt


def _run(layout, lg, t, w_dice, dloss=None, argmax=False):
    """fwd -> finalize -> bwd through the C ABI: ([loss, ce, dice], dlogits as NCHW float64, partial rows, argmax)"""
    L = _L()
    lib = L.lib()
    if layout == "nchw_f32":
        n, c, h, w = lg.shape
    else:
        n, h, w, c = lg.shape
    lay = L.SEG_NCHW if layout == "nchw_f32" else L.SEG_NHWC
    dt = L.DT_BF16 if lg.dtype == torch.bfloat16 else L.DT_F32
    d = L.HeadDesc(dt, n, h, w, 1, c)
    nb = lib.oct_seg_loss_blocks(n * h * w, c)
    part = torch.full((nb, L.HEAD_LOSS_SLOTS), float("nan"), dtype=torch.float64, device="cuda")
    amax = torch.full((n, h, w), -7, dtype=torch.int64, device="cuda") if argmax else None
    out = torch.empty(3, device="cuda")
    coef = torch.empty(2 * L.MAX_CLASSES, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.oct_seg_loss_forward(C.byref(d), lay, lg.data_ptr(), t.data_ptr(), L.ptr(amax), part.data_ptr(), st))
    L.check(lib.oct_head_loss_finalize(C.byref(d), part.data_ptr(), nb, 1.0, w_dice, 1e-7, out.data_ptr(), coef.data_ptr(), st))
    dl = torch.full_like(lg, float("nan"))
    L.check(lib.oct_seg_loss_backward(C.byref(d), lay, lg.data_ptr(), t.data_ptr(), coef.data_ptr() if w_dice else None, 1.0,
                                      L.ptr(dloss), dl.data_ptr(), None, st))
    dln = dl.float() if layout == "nchw_f32" else dl.float().permute(0, 3, 1, 2)
    return out.cpu().numpy(), dln.cpu().double().numpy(), part, amax


def _bf16_ulp(v):
    a = np.maximum(np.abs(v), np.finfo(np.float32).tiny)
    return np.exp2(np.floor(np.log2(a)) - 7)


@pytest.mark.parametrize("shape", [(3, 37, 53), (4, 496, 768)])
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
@pytest.mark.parametrize("classes", [1, 2, 3, 8, 9, 10, 11, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernels_match_the_float64_oracle(layout, classes, w_dice, shape):
    bf16 = layout == "nhwc_bf16"
    x, t = _logits(shape, classes, bf16)
    ref, rdl = _oracle(shape, classes, bf16, w_dice)
    lg, td = _device_logits(layout, x), torch.from_numpy(t).cuda()
    got, dl, part, _ = _run(layout, lg, td, w_dice)
    assert not torch.isnan(part).any()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-7)
    scale = float(np.abs(rdl).max())
    err = np.abs(dl - rdl)
    if bf16:
        assert (err <= np.maximum(_bf16_ulp(rdl), 1e-6 * scale)).all(), float((err / _bf16_ulp(rdl)).max())
    else:
        assert err.max() <= 1e-5 * scale, (err.max(), scale)
    # deterministic: a second run gives the same bits
    got2, dl2, part2, _ = _run(layout, lg, td, w_dice)
    assert np.array_equal(got, got2) and np.array_equal(dl, dl2) and torch.equal(part, part2)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_upstream_gradient_bad_label_and_argmax(layout):
    shape, classes = (3, 37, 53), 5
    x, t = _logits(shape, classes, layout == "nhwc_bf16")
    x = x.copy()
    x[1, 2, 4, 7] = x[1, 3, 4, 7] = x[1, :, 4, 7].max() + 1.0     # a tie: the first maximum wins
    lg, td = _device_logits(layout, x), torch.from_numpy(t).cuda()
    _, dl1, _, amax = _run(layout, lg, td, 0.7, argmax=True)
    assert np.array_equal(amax.cpu().numpy(), x.argmax(1)) and int(amax[1, 4, 7]) == 2
    g = torch.tensor([0.25], device="cuda")
    _, dlg, _, _ = _run(layout, lg, td, 0.7, dloss=g)
    np.testing.assert_allclose(dlg, 0.25 * dl1, rtol=1e-6 if layout != "nhwc_bf16" else 1e-2, atol=0)
    bad = td.clone()
    bad[0, 0, 0] = classes
    assert np.isnan(_run(layout, lg, bad, 0.0)[0][0])
    bad[0, 0, 0] = -1
    assert np.isnan(_run(layout, lg, bad, 0.7)[0][0])
    # pure predict: no target, no partial rows
    L = _L()
    n, h, w = shape
    d = L.HeadDesc(L.DT_BF16 if lg.dtype == torch.bfloat16 else L.DT_F32, n, h, w, 1, classes)
    a2 = torch.full((n, h, w), -7, dtype=torch.int64, device="cuda")
    L.check(L.lib().oct_seg_loss_forward(C.byref(d), L.SEG_NCHW if layout == "nchw_f32" else L.SEG_NHWC, lg.data_ptr(), None,
                                         a2.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(a2, amax)


def test_cross_entropy_dice_is_f_cross_entropy_and_differentiates():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    x, t = _logits((3, 37, 53), 4, False)
    a = torch.from_numpy(x).float().cuda().requires_grad_(True)
    b = a.detach().clone().requires_grad_(True)
    td = torch.from_numpy(t).cuda()
    la = cross_entropy_dice(a, td)
    lb = F.cross_entropy(b, td)
    assert la.dim() == 0 and la.requires_grad
    (2.0 * la).backward()
    (2.0 * lb).backward()
    np.testing.assert_allclose(float(la.detach()), float(lb.detach()), rtol=1e-6)
    assert float((a.grad - b.grad).abs().max()) <= 1e-6 * float(b.grad.abs().max())
    ref, rdl = _oracle((3, 37, 53), 4, False, 0.7)
    c = torch.from_numpy(x).float().cuda().requires_grad_(True)
    lc = cross_entropy_dice(c, td, 1.0, 0.7)
    lc.backward()
    np.testing.assert_allclose(float(lc.detach()), ref[0], rtol=1e-5)
    assert float(np.abs(c.grad.double().cpu().numpy() - rdl).max()) <= 1e-5 * float(np.abs(rdl).max())


@pytest.mark.parametrize("w_dice", [0.0, 0.5])
def test_functional_loss_matches_the_fused_unet_head(w_dice):
    """two implementations of one definition: cross_entropy_dice on UNet's logits == UNet.loss (fp32 mode)"""
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    torch.manual_seed(0)
    m = UNet(1, 4, init_features=8, compute_dtype="f32").cuda().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 1, 32, 48, generator=g).cuda()
    t = torch.randint(0, 4, (2, 32, 48), generator=g).cuda()
    a = float(cross_entropy_dice(m.logits(x), t, 1.0, w_dice))
    b = m.loss(x, t, 1.0, w_dice).cpu().numpy()
    np.testing.assert_allclose(a, b[0], rtol=1e-6)


# ---- the networks ----------------------------------------------------------------------------------------------------
SD = [("attunet_c3_2x32x48", "AttU_Net", dict(channels=[4, 8, 16, 32, 64])), ("sd_unet_c2_1x32x32", "U_Net", {}),
      ("attunet4_c3_2x24x40", "AttU_Net4", dict(channels=[4, 8, 16, 32]))]
MG = [("mgunet2_c3_2x48x64", "MGUNet_2"), ("mgunet_c2_2x160x192", "MGUNet")]
RELAY = ["relaynet_c4_f8_2x32x48", "relaynet_in3_c9_f16_1x16x40"]


def _close(got, ref, key, rel, floor=1e-4):
    ref = np.asarray(ref, np.float64)
    tol = rel * max(float(np.abs(ref).max()), floor)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    assert err <= tol, f"{key}: max err {err:.3e} > {tol:.3e}"


def _fixture_model(golden_dir, name):
    """(z, model in f32 train mode on the device, x, t) the way the existing fixture tests build each network"""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    if name.startswith("relaynet"):
        from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.ReLayNet_2017 import ReLayNet
        seed, n, cin, ncls, nf, h, w = (int(v) for v in z["meta"])
        m = ReLayNet(in_channels=cin, num_classes=ncls, num_filters=nf, compute_dtype="f32")
        m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w0/")}, strict=True)
        return z, m.cuda().train(), torch.from_numpy(z["x"]), torch.from_numpy(z["target"])
    seed, n, cin, ncls, h, w = (int(v) for v in z["meta"])
    sd = {k: (c, kw) for k, c, kw in SD}
    if name in sd:
        from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net import unet as U
        cls, kw = sd[name]
        ctor = lambda ci, nc: getattr(U, cls)(ci, nc, compute_dtype="f32", **kw)   # noqa: E731
    else:
        from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
        cls = dict(MG)[name]
        ctor = lambda ci, nc: getattr(M, cls)(ci, nc, feature_scale=16, compute_dtype="f32")   # noqa: E731
    m, x, t = bio_case(ctor, seed, n, cin, ncls, h, w)
    assert bio_weights_match(z, m.state_dict())
    return z, m.cuda().train(), x, t


@pytest.mark.parametrize("name", [k for k, _, _ in SD] + [k for k, _ in MG] + RELAY)
def test_f32_forward_backward_matches_reference_fixture(golden_dir, name):
    z, m, x, t = _fixture_model(golden_dir, name)
    out = m.forward_backward(x.cuda(), t.cuda())
    assert out.shape == (3,) and out.device.type == "cuda"
    loss = out.cpu().numpy()
    np.testing.assert_allclose(loss[0], float(z["loss"][0]), rtol=2e-5)
    np.testing.assert_allclose(loss[1], loss[0], rtol=0)
    assert loss[2] == 0.0
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    if name.startswith("relaynet"):
        for k, g in grads.items():
            _close(g, z["g/" + k], k, 2e-3)
    else:
        assert bio_grad_errors(z, grads, 2e-3) == []
    sd = m.state_dict()
    for k in z.files:
        if k.startswith("b1/") and "running" in k:
            _close(sd[k[3:]].cpu().numpy(), z[k], k, 1e-4)
    nbt = [k for k in sd if k.endswith("num_batches_tracked")]
    assert nbt and all(int(sd[k]) == 1 for k in nbt)        # one forward's worth


def _sd_net(cls, dtype, kw, cin=1, classes=3, seed=11):
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net import unet as U
    torch.manual_seed(seed)
    return getattr(U, cls)(cin, classes, compute_dtype=dtype, **kw).cuda().train()


# gradients summed with fp32 atomics (oct_channel_sum: convolutions without BatchNorm whose Cin is not a multiple of 32),
# as listed by test_gpu_blocks.py's deterministic-schedule test: equal up to summation order
LOOSE = ("Conv_1x1.bias", "Conv1.init_conv.bias", "Conv2.init_conv.bias")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cls,kw,shape", [("AttU_Net", dict(channels=[16, 32, 64, 128, 256]), (2, 1, 32, 48)),
                                          ("U_Net", {}, (1, 1, 32, 32))])
def test_forward_backward_equals_the_functional_path(dtype, cls, kw, shape):
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    m = _sd_net(cls, dtype, kw)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g).cuda()
    t = torch.randint(0, 3, (shape[0], shape[2], shape[3]), generator=g).cuda()
    init = {k: v.clone() for k, v in m.state_dict().items()}
    e = ops.kernels(dtype)
    keep = e.deterministic
    res = {}
    try:
        e.deterministic = True
        m.zero_grad(set_to_none=True)
        loss = cross_entropy_dice(m(x), t)
        loss.backward()
        res["functional"] = ({k: p.grad.clone() for k, p in m.named_parameters()}, float(loss.detach()))
        m.load_state_dict(init)
        out = m.forward_backward(x, t)
        res["fused"] = ({k: p.grad.clone() for k, p in m.named_parameters()}, float(out[0]))
    finally:
        e.deterministic = keep
    a, b = res["functional"][0], res["fused"][0]
    bad = [k for k in a if not (torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-7) if k in LOOSE else torch.equal(a[k], b[k]))]
    assert bad == [], bad
    assert res["functional"][1] == res["fused"][1]


def test_forward_backward_contracts():
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    m = _sd_net("AttU_Net", "f32", dict(channels=[16, 32, 64, 128, 256]))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 1, 32, 48, generator=g).cuda()
    t = torch.randint(0, 3, (2, 32, 48), generator=g).cuda()
    init = {k: v.clone() for k, v in m.state_dict().items()}
    e = ops.kernels("f32")
    keep = e.deterministic
    try:
        e.deterministic = True
        m.forward_backward(x, t, 1.0, 0.5)
        g1 = {k: p.grad.clone() for k, p in m.named_parameters()}
        m.load_state_dict(init)
        ids = {k: id(p.grad) for k, p in m.named_parameters()}
        l2 = m.forward_backward(x, t, 1.0, 0.5)          # overwrites, does not accumulate; same tensors
        for k, p in m.named_parameters():
            assert id(p.grad) == ids[k]
            assert torch.allclose(p.grad, g1[k], rtol=1e-4, atol=1e-7) if k in LOOSE else torch.equal(p.grad, g1[k]), k
        assert float(l2[2]) > 0.0                          # the Dice term is there
        # loss() in train mode: the loss forward_backward returned
        m.load_state_dict(init)
        l3 = m.loss(x, t, 1.0, 0.5)
        assert torch.equal(l3, l2)
    finally:
        e.deterministic = keep
    # predict == model(x).argmax(1), in both modes
    for mode in (True, False):
        m.train(mode)
        with torch.no_grad():
            ref = m(x).argmax(1)
        m.train(mode)
        assert torch.equal(m.predict(x), ref)
    m.train()
    # FusedSGD keeps the flat views: forward_backward writes into them
    opt = FusedSGD(list(m.named_parameters()), lr=0.01, momentum=0.9)
    for _ in range(2):
        m.forward_backward(x, t)
        opt.step()
    for (k, p), o in zip(m.named_parameters(), opt.layout.offsets):
        assert p.grad.data_ptr() == opt.flat_g[o:].data_ptr(), k
    assert float(opt.flat_g.abs().sum()) > 0
    with pytest.raises(RuntimeError, match="needs train"):
        m.eval().forward_backward(x, t)
    big = _sd_net("AttU_Net", "f32", dict(channels=[16, 32, 64, 128, 256]), classes=17)
    with pytest.raises(NotImplementedError, match="16 classes"):
        big.forward_backward(x, t)


def test_data_parallel_trainer_runs_the_logits_networks():
    """world size 1, deterministic: two DataParallelTrainer steps == forward_backward + FusedSGD.step by hand.  The biases
    whose gradients are atomics-summed (LOOSE) are frozen in both runs, so step 2 starts from equal parameters."""
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp, ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 1, 32, 48, generator=g).cuda()
    t = torch.randint(0, 3, (2, 32, 48), generator=g).cuda()
    e = ops.kernels("f32")
    keep = e.deterministic
    res = []
    try:
        e.deterministic = True
        for by_hand in (False, True):
            m = _sd_net("AttU_Net", "f32", dict(channels=[16, 32, 64, 128, 256]), seed=12)
            for k, p in m.named_parameters():
                p.requires_grad_(k not in LOOSE)
            if by_hand:
                opt = FusedSGD(list(m.named_parameters()), lr=0.01, momentum=0.9)
                for _ in range(2):
                    m.forward_backward(x, t, 1.0, 0.3)
                    opt.step()
            else:
                tr = ddp.DataParallelTrainer(m, lr=0.01, momentum=0.9, w_dice=0.3)
                assert tr.reducer.buckets == [(0, 0, tr.opt.flat_g.numel())]
                for _ in range(2):
                    tr.step(x, t)
            res.append({k: p.detach().clone() for k, p in m.named_parameters()})
    finally:
        e.deterministic = keep
    bad = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
    assert bad == [], bad
    moved = _sd_net("AttU_Net", "f32", dict(channels=[16, 32, 64, 128, 256]), seed=12)
    assert not torch.equal(moved.Conv1.init_conv.weight.cuda(), res[0]["Conv1.init_conv.weight"])


def test_full_size_cfg4_attunet_bf16():
    """cfg4 AttU_Net(1, 3) at 2 x 496 x 768, production dtype: finite, and the F.cross_entropy path's loss"""
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net.unet import AttU_Net
    torch.manual_seed(0)
    m = AttU_Net(1, 3).cuda().train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 1, 496, 768, generator=g).cuda()
    t = torch.randint(0, 3, (2, 496, 768), generator=g).cuda()
    out = m.forward_backward(x, t)
    assert torch.isfinite(out).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    with torch.no_grad():
        ref = float(F.cross_entropy(m(x), t))
    assert abs(float(out[0]) - ref) <= 3e-2 * max(1.0, abs(ref)), (float(out[0]), ref)
