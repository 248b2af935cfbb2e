"""GPU: the weighted CE + soft-Dice loss (class weights, pixel weight map, ignore_index) -- the oct_seg_loss_*_weighted kernels
against the float64 reference of tests/test_seg_loss_weighted_cpu.py, the functional loss against F.cross_entropy(weight=,
ignore_index=), and forward_backward / loss / DataParallelTrainer of the networks against the same network stepped through
autograd with torch's weighted loss.  Bounds are those of tests/test_gpu_seg_loss.py, over all elements."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_seg_loss import LAYOUTS, LOOSE, _bf16_ulp, _close, _device_logits, _fixture_model, _logits, _sd_net
from test_seg_loss_weighted_cpu import reference_loss, weighted_case

pytestmark = pytest.mark.gpu

OPTS = ["class", "map", "ignore", "all"]


def _L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    return _lib


def _ignore_value(classes, opts):
    return -100 if (classes + (opts == "all")) % 2 else 255


@functools.lru_cache(maxsize=2)
def _case(shape, classes, bf16, opts):
    """logits and labels as test_gpu_seg_loss.py seeds them, plus the options of this case: (x, t, cw, pw, ig, ignored mask)"""
    x, t = _logits(shape, classes, bf16)
    ig = _ignore_value(classes, opts)
    cw, pw, ign = weighted_case(shape, classes, classes * 1000 + shape[1] + 7, ig)
    if opts in ("ignore", "all"):
        t = np.where(ign, ig, t)
    else:
        ig, ign = None, np.zeros_like(ign)
    return x, t, cw if opts in ("class", "all") else None, pw if opts in ("map", "all") else None, ig, ign


@functools.lru_cache(maxsize=2)
def _reference(shape, classes, bf16, opts, w_dice):
    x, t, cw, pw, ig, _ = _case(shape, classes, bf16, opts)
    return reference_loss(x, t, 1.0, w_dice, 1e-7, cw, pw, ig)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(layout, lg, t, w_dice, cw=None, pw=None, ig=None, dloss=None, ce_only=False):
    """The weighted kernels through the C ABI: ([loss, ce, dice], dlogits as NCHW float64, partial rows, sum omega).
    ce_only: weight_sum -> backward (writes the CE rows) -> finalize; else forward -> finalize -> backward."""
    L = _L()
    lib = L.lib()
    if layout == "nchw_f32":
        n, c, h, w = lg.shape
    else:
        n, h, w, c = lg.shape
    lay = L.SEG_NCHW if layout == "nchw_f32" else L.SEG_NHWC
    d = L.HeadDesc(L.DT_BF16 if lg.dtype == torch.bfloat16 else L.DT_F32, n, h, w, 1, c)
    nb = lib.oct_seg_loss_blocks(n * h * w, c)
    part = torch.full((nb, L.HEAD_LOSS_SLOTS), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.empty(3, device="cuda")
    coef = torch.empty(2 * L.MAX_CLASSES, device="cuda")
    wsum = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    dl = torch.full_like(lg, float("nan"))
    st = torch.cuda.current_stream().cuda_stream
    has, igv = int(ig is not None), int(ig or 0)
    if ce_only:
        scratch = torch.full((nb,), float("nan"), dtype=torch.float64, device="cuda")
        L.check(lib.oct_seg_loss_weight_sum(C.byref(d), t.data_ptr(), L.ptr(cw), L.ptr(pw), has, igv, scratch.data_ptr(),
                                            wsum.data_ptr(), st))
        L.check(lib.oct_seg_loss_backward_weighted(C.byref(d), lay, lg.data_ptr(), t.data_ptr(), L.ptr(cw), L.ptr(pw), has, igv,
                                                   wsum.data_ptr(), None, 1.0, L.ptr(dloss), dl.data_ptr(), part.data_ptr(), st))
        L.check(lib.oct_seg_loss_finalize_weighted(C.byref(d), part.data_ptr(), nb, 1.0, 0.0, 1e-7, out.data_ptr(),
                                                   coef.data_ptr(), None, st))
    else:
        L.check(lib.oct_seg_loss_forward_weighted(C.byref(d), lay, lg.data_ptr(), t.data_ptr(), L.ptr(cw), L.ptr(pw), has, igv,
                                                  part.data_ptr(), st))
        L.check(lib.oct_seg_loss_finalize_weighted(C.byref(d), part.data_ptr(), nb, 1.0, w_dice, 1e-7, out.data_ptr(),
                                                   coef.data_ptr(), wsum.data_ptr(), st))
        L.check(lib.oct_seg_loss_backward_weighted(C.byref(d), lay, lg.data_ptr(), t.data_ptr(), L.ptr(cw), L.ptr(pw), has, igv,
                                                   wsum.data_ptr(), coef.data_ptr() if w_dice else None, 1.0, L.ptr(dloss),
                                                   dl.data_ptr(), None, st))
    dln = dl.float() if layout == "nchw_f32" else dl.float().permute(0, 3, 1, 2)
    return out.cpu().numpy(), dln.cpu().double().numpy(), part, wsum


def _check_gradient(dl, rdl, bf16, ign):
    scale = float(np.abs(rdl).max())
    err = np.abs(dl - rdl)
    print(f"gradient: max err {err.max():.3e}, max |ref| {scale:.3e}, ratio {err.max() / scale:.3e}")
    if bf16:
        assert (err <= np.maximum(_bf16_ulp(rdl), 1e-6 * scale)).all(), float((err / _bf16_ulp(rdl)).max())
    else:
        assert err.max() <= 1e-5 * scale, (err.max(), scale)
    assert (dl.transpose(0, 2, 3, 1)[ign] == 0).all()          # exactly 0 in every class of an ignored pixel


# layout varies fastest: the float64 reference of a case is computed once for the layouts that share it
KERNEL_CASES = [pytest.param(layout, classes, w_dice, shape, opts, id=f"{layout}-c{classes}-dice{w_dice}-{shape[1]}x{shape[2]}-{opts}")
                for shape, classes, opts, w_dice, layout in itertools.product(
                    [(3, 37, 53), (4, 496, 768)], [2, 3, 9, 16], OPTS, [0.0, 0.7], ["nhwc_f32", "nchw_f32", "nhwc_bf16"])]


@pytest.mark.parametrize("layout,classes,w_dice,shape,opts", KERNEL_CASES)
def test_weighted_kernels_match_the_float64_reference(layout, classes, w_dice, shape, opts):
    bf16 = layout == "nhwc_bf16"
    x, t, cw, pw, ig, ign = _case(shape, classes, bf16, opts)
    ref, rdl = _reference(shape, classes, bf16, opts, w_dice)
    lg, td, cwd, pwd = _device_logits(layout, x), _dev(t), _dev(cw), _dev(pw)
    got, dl, part, wsum = _run(layout, lg, td, w_dice, cwd, pwd, ig)
    print(f"loss {got} reference {ref}")
    assert not torch.isnan(part).any()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-7)
    _check_gradient(dl, rdl, bf16, ign)
    # deterministic: a second run gives the same bits
    got2, dl2, part2, wsum2 = _run(layout, lg, td, w_dice, cwd, pwd, ig)
    assert np.array_equal(got, got2) and np.array_equal(dl, dl2) and torch.equal(part, part2) and torch.equal(wsum, wsum2)
    if w_dice == 0.0:
        # the schedule of a CE-only training step: sum omega from the labels and the map, the logits read once
        got3, dl3, part3, wsum3 = _run(layout, lg, td, 0.0, cwd, pwd, ig, ce_only=True)
        assert not torch.isnan(part3).any()
        np.testing.assert_allclose(got3[:2], ref[:2], rtol=1e-5, atol=1e-7)
        assert got3[2] == 0.0
        _check_gradient(dl3, rdl, bf16, ign)
        assert torch.equal(wsum3, wsum)                         # one reduction order: the two schedules agree to the bit
        got4, dl4, part4, _ = _run(layout, lg, td, 0.0, cwd, pwd, ig, ce_only=True)
        assert np.array_equal(got3, got4) and np.array_equal(dl3, dl4) and torch.equal(part3, part4)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_other_bad_labels_are_nan_and_everything_ignored_is_nan(layout):
    shape, classes = (3, 37, 53), 5
    x, t = _logits(shape, classes, layout == "nhwc_bf16")
    lg = _device_logits(layout, x)
    td = torch.from_numpy(t).cuda()
    td[1, :5] = 255
    for ce_only in (False, True):
        assert np.isfinite(_run(layout, lg, td, 0.0, ig=255, ce_only=ce_only)[0]).all()
        for badv in (classes, -1, -100):
            bad = td.clone()
            bad[2, 3, 4] = badv
            out, _, _, _ = _run(layout, lg, bad, 0.0 if ce_only else 0.7, ig=255, ce_only=ce_only)
            assert np.isnan(out[0]) and np.isnan(out[1]), (badv, out)
            # ... and the same label is fine once it is the ignored one
            if badv < 0:
                bad[td == 255] = badv
                assert np.isfinite(_run(layout, lg, bad, 0.0 if ce_only else 0.7, ig=badv, ce_only=ce_only)[0]).all()
        # ignore_index None: the ignored value is a bad label like any other
        assert np.isnan(_run(layout, lg, td, 0.0, ce_only=ce_only)[0][0])
        # everything ignored: 0 / 0 = NaN as torch; nothing faults, every gradient is exactly 0
        gone = torch.full_like(td, -100)
        out, dl, part, wsum = _run(layout, lg, gone, 0.0 if ce_only else 0.7, ig=-100, ce_only=ce_only)
        assert np.isnan(out[0]) and np.isnan(out[1]) and float(wsum) == 0.0
        assert not torch.isnan(part).any() and (dl == 0).all()
    assert torch.isnan(F.cross_entropy(torch.zeros(1, 3, 2, 2), torch.full((1, 2, 2), -100)))      # what torch does


@pytest.mark.parametrize("w_dice", [0.0, 0.7])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_options_give_the_unweighted_loss(layout, w_dice):
    from test_gpu_seg_loss import _run as run_plain
    shape, classes = (3, 37, 53), 9
    x, t = _logits(shape, classes, layout == "nhwc_bf16")
    lg, td = _device_logits(layout, x), torch.from_numpy(t).cuda()
    ref, rdl, _, _ = run_plain(layout, lg, td, w_dice)
    ones_c = torch.ones(classes, device="cuda")
    ones_p = torch.ones(shape, device="cuda")
    for kw in (dict(cw=ones_c), dict(pw=ones_p), dict(ig=255), dict(cw=ones_c, pw=ones_p, ig=-100)):
        got, dl, _, wsum = _run(layout, lg, td, w_dice, **kw)
        assert float(wsum) == float(np.prod(shape))
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
        np.testing.assert_allclose(dl, rdl, rtol=1e-6, atol=0)     # omega / sum(omega) is 1 / N: last-bit differences at most


def test_functional_loss_with_no_options_runs_the_unweighted_kernels():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice, loss_and_dlogits
    x, t = _logits((3, 37, 53), 4, False)
    td = torch.from_numpy(t).cuda()
    res = []
    for kw in ({}, dict(class_weight=None, pixel_weight=None, ignore_index=None)):
        a = torch.from_numpy(x).float().cuda().requires_grad_(True)
        la = cross_entropy_dice(a, td, 1.0, 0.7, **kw)
        la.backward()
        res.append((la.detach().clone(), a.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    nhwc = torch.from_numpy(x).float().cuda().permute(0, 2, 3, 1).contiguous()
    for wd in (0.0, 0.7):
        o1, d1 = loss_and_dlogits(nhwc, td, 1.0, wd)
        o2, d2 = loss_and_dlogits(nhwc, td, 1.0, wd, class_weight=None, pixel_weight=None, ignore_index=None)
        assert torch.equal(o1, o2) and torch.equal(d1, d2)


@pytest.mark.parametrize("ig", [-100, 255])
def test_cross_entropy_dice_is_weighted_f_cross_entropy(ig):
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    shape, classes = (3, 37, 53), 4
    x, t = _logits(shape, classes, False)
    cw, pw, ign = weighted_case(shape, classes, 21, ig)
    td = torch.from_numpy(np.where(ign, ig, t)).cuda()
    cwd, pwd = _dev(cw), _dev(pw)
    a = torch.from_numpy(x).float().cuda().requires_grad_(True)
    b = a.detach().clone().requires_grad_(True)
    la = cross_entropy_dice(a, td, class_weight=cwd, ignore_index=ig)
    lb = F.cross_entropy(b, td, weight=cwd, ignore_index=ig)
    assert la.dim() == 0 and la.requires_grad
    (2.0 * la).backward()
    (2.0 * lb).backward()
    np.testing.assert_allclose(float(la.detach()), float(lb.detach()), rtol=1e-6)
    assert float((a.grad - b.grad).abs().max()) <= 1e-6 * float(b.grad.abs().max())
    assert (a.grad.permute(0, 2, 3, 1)[torch.from_numpy(ign).cuda()] == 0).all()
    # a sequence of floats is the same weights; with a map: torch's per-pixel loss times the map over sum omega
    c = a.detach().clone().requires_grad_(True)
    e = a.detach().clone().requires_grad_(True)
    lc = cross_entropy_dice(c, td, class_weight=[float(v) for v in cw], pixel_weight=pwd, ignore_index=ig)
    valid = td != ig
    omega = valid.float() * cwd[torch.where(valid, td, 0)] * pwd
    le = (F.cross_entropy(e, td, weight=cwd, ignore_index=ig, reduction="none") * pwd).sum() / omega.sum()
    (2.0 * lc).backward()
    (2.0 * le).backward()
    np.testing.assert_allclose(float(lc.detach()), float(le.detach()), rtol=1e-6)
    assert float((c.grad - e.grad).abs().max()) <= 1e-6 * float(e.grad.abs().max())
    # with a Dice term: the float64 reference
    ref, rdl = reference_loss(x, td.cpu().numpy(), 1.0, 0.7, 1e-7, cw, pw, ig)
    f = a.detach().clone().requires_grad_(True)
    lf = cross_entropy_dice(f, td, 1.0, 0.7, class_weight=cwd, pixel_weight=pwd, ignore_index=ig)
    lf.backward()
    np.testing.assert_allclose(float(lf.detach()), ref[0], rtol=1e-5)
    assert float(np.abs(f.grad.double().cpu().numpy() - rdl).max()) <= 1e-5 * float(np.abs(rdl).max())


# ---- the networks ----------------------------------------------------------------------------------------------------------
def _options_for(t, classes, seed, ig):
    """(labels with some overwritten by ig, class weights, map) on the device for a fixture's target"""
    cw, pw, ign = weighted_case(tuple(t.shape), classes, seed, ig)
    ign[0] = np.random.default_rng(seed).random(ign.shape[1:]) < 0.3      # a fixture has 1-2 images: keep most of image 0
    return torch.from_numpy(np.where(ign, ig, t.numpy())).cuda(), _dev(cw), _dev(pw)


def _torch_weighted(out, t, cw, pw, ig, probs=False):
    """torch's loss: (F.cross_entropy(weight=, ignore_index=, reduction='none') * map).sum() / sum omega"""
    valid = t != ig
    omega = valid.float() * cw[torch.where(valid, t, 0)] * pw
    per = (F.nll_loss(torch.log(out), t, weight=cw, ignore_index=ig, reduction="none") if probs
           else F.cross_entropy(out, t, weight=cw, ignore_index=ig, reduction="none"))
    return (per * pw).sum() / omega.sum()


def _engine_fixture(golden_dir, name):
    """(model in f32 train mode on the device, x, t, classes): BioUNet and UNet as their fixture tests build them"""
    if name.startswith("bionet"):
        from oracle.cases import bio_case
        from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.BioNet_2020 import UNet
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        seed, n, cin, ncls, h, w = (int(v) for v in z["meta"])
        m, x, t = bio_case(lambda a, b: UNet(a, b, compute_dtype="f32"), seed, n, cin, ncls, h, w)
        return m.cuda().train(), x, t, ncls
    from test_gpu_unet import load
    z, m = load(golden_dir, name, "f32")
    return m, torch.from_numpy(z["x"]), torch.from_numpy(z["target"]), int(z["meta"][1])


# Both sides of the network comparison below are fp32 runs on the device, so a gradient that is analytically zero is rounding
# noise on BOTH, of the size of an ulp of the gradients it cancels out of, and the 2e-3 relative bound says nothing about it.
# oracle/cases.py::bio_grad_errors has the project's rule for that (a conv bias in front of a train-mode BatchNorm: "zero up to
# rounding on both sides", both below 1e-6), and it is applied here by value instead of by name because the fixtures hold one
# more such case: MGUNet_2 at 2 x 48 x 64 pools its 5 x 5 branch to ONE pixel, BatchNorm over the two images' values returns
# +-1 whatever they are, and every gradient in front of it (mgb.conv3_1's BatchNorm) is O(eps).  Measured there: torch-loss
# side 4.5e-8, HIP-loss side within 2.4e-7 of it, each equal to the bit on a second run.
ZERO_UP_TO_ROUNDING = 1e-6

NETS = ["attunet_c3_2x32x48", "mgunet2_c3_2x48x64", "relaynet_c4_f8_2x32x48", "bionet_unet_c2_2x16x24", "unet_c8_f4_2x32x32"]


def _two_copies(golden_dir, name):
    if name.startswith(("bionet", "unet")):
        a, x, t, ncls = _engine_fixture(golden_dir, name)
        b = _engine_fixture(golden_dir, name)[0]
    else:
        _, a, x, t = _fixture_model(golden_dir, name)
        b = _fixture_model(golden_dir, name)[1]
        ncls = a._classes()
    return a, b, x, t, ncls


@pytest.mark.parametrize("ig", [-100, 255])
@pytest.mark.parametrize("name", NETS)
def test_f32_weighted_forward_backward_matches_torch_loss_through_autograd(golden_dir, name, ig):
    a, b, x, t, ncls = _two_copies(golden_dir, name)
    xd = x.cuda()
    td, cw, pw = _options_for(t, ncls, 31, ig)
    out = a.forward_backward(xd, td, class_weight=cw, pixel_weight=pw, ignore_index=ig)
    assert out.shape == (3,) and out.device.type == "cuda"
    ref = _torch_weighted(b(xd), td, cw, pw, ig, probs=name.startswith("unet"))
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
    assert nbt and all(int(sa[k]) == 1 and int(sb[k]) == 1 for k in nbt)


@pytest.mark.parametrize("w_dice", [0.0, 0.5])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_weighted_forward_backward_equals_the_functional_path(dtype, w_dice):
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    m = _sd_net("AttU_Net", dtype, dict(channels=[16, 32, 64, 128, 256]))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 32, 48, generator=g).cuda()
    td, cw, pw = _options_for(torch.randint(0, 3, (2, 32, 48), generator=g), 3, 32, 255)
    kw = dict(class_weight=cw, pixel_weight=pw, ignore_index=255)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    e = ops.kernels(dtype)
    keep = e.deterministic
    res = {}
    try:
        e.deterministic = True
        m.zero_grad(set_to_none=True)
        loss = cross_entropy_dice(m(x), td, 1.0, w_dice, **kw)
        loss.backward()
        res["functional"] = ({k: p.grad.clone() for k, p in m.named_parameters()}, float(loss.detach()))
        m.load_state_dict(init)
        out = m.forward_backward(x, td, 1.0, w_dice, **kw)
        res["fused"] = ({k: p.grad.clone() for k, p in m.named_parameters()}, float(out[0]))
    finally:
        e.deterministic = keep
    a, b = res["functional"][0], res["fused"][0]
    bad = [k for k in a if not (torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-7) if k in LOOSE else torch.equal(a[k], b[k]))]
    assert bad == [], bad
    assert res["functional"][1] == res["fused"][1]
    assert float(out[2]) > 0.0 if w_dice else float(out[2]) == 0.0


def _small_unet(seed=50):
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    torch.manual_seed(seed)
    return UNet(1, 4, init_features=8, compute_dtype="f32").cuda().train()


def _small_data(classes, seed, ig=255):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 1, 32, 48, generator=g).cuda()
    td, cw, pw = _options_for(torch.randint(0, classes, (2, 32, 48), generator=g), classes, seed, ig)
    return x, td, dict(class_weight=cw, pixel_weight=pw, ignore_index=ig)


@pytest.mark.parametrize("net", ["UNet", "AttU_Net"])
def test_weighted_forward_backward_contracts(net):
    from retinal_oct_image_segmentation_via_deep_learning_amd import ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    engine = net == "UNet"
    m = _small_unet() if engine else _sd_net("AttU_Net", "f32", dict(channels=[16, 32, 64, 128, 256]))
    x, td, kw = _small_data(4 if engine else 3, 6)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    e = ops.kernels("f32")
    keep = e.deterministic
    try:
        e.deterministic = True
        for w_dice in (0.0, 0.5):
            m.load_state_dict(init)
            l1 = m.forward_backward(x, td, 1.0, w_dice, **kw)
            sd = m.state_dict()
            nbt = [k for k in sd if k.endswith("num_batches_tracked")]
            assert nbt and all(int(sd[k]) == 1 for k in nbt)                 # one forward's worth
            ids = {k: id(p.grad) for k, p in m.named_parameters()}
            stats = {k: v.clone() for k, v in sd.items() if "running" in k}
            # the same buffers as a step on the unweighted (fused-head) route: BatchNorm moves once, by the same batch statistics
            m.load_state_dict(init)
            m.forward_backward(x, td.clamp(0, 2), 1.0, w_dice)
            sd = m.state_dict()
            assert all(int(sd[k]) == 1 for k in nbt) and all(torch.equal(sd[k], v) for k, v in stats.items())
            for k, p in m.named_parameters():
                assert id(p.grad) == ids[k]                                   # overwritten in place, same tensors
            # loss() in train mode: the loss forward_backward returned
            m.load_state_dict(init)
            l3 = m.loss(x, td, 1.0, w_dice, **kw)
            if w_dice:
                assert torch.equal(l3, l1) and float(l1[2]) > 0.0
            else:
                assert torch.equal(l3[:2], l1[:2]) and float(l1[2]) == 0.0   # a CE-only step does not accumulate the Dice sums
    finally:
        e.deterministic = keep
    # FusedSGD keeps the flat views: the weighted route writes into them
    m.load_state_dict(init)
    opt = FusedSGD(list(m.named_parameters()), lr=0.01, momentum=0.9)
    for _ in range(2):
        m.forward_backward(x, td, **kw)
        opt.step()
    for (k, p), o in zip(m.named_parameters(), opt.layout.offsets):
        assert p.grad.data_ptr() == opt.flat_g[o:].data_ptr(), k
    assert float(opt.flat_g.abs().sum()) > 0 and bool(torch.isfinite(opt.flat_g).all())
    with pytest.raises(RuntimeError, match="needs train"):
        m.eval().forward_backward(x, td, **kw)


def test_unet_want_probs_and_stage_hook_on_the_weighted_route():
    m = _small_unet()
    x, td, kw = _small_data(4, 9)
    init = {k: v.clone() for k, v in m.state_dict().items()}

    class Hook:
        flush_stages = set(range(len(m._engine.backward_stages())))

        def __init__(self):
            self.seen = []

        def stage_done(self, idx):
            self.seen.append(idx)

    hook = Hook()
    out, probs = m.forward_backward(x, td, want_probs=True, stage_hook=hook, **kw)
    assert hook.seen == sorted(Hook.flush_stages)
    m.load_state_dict(init)
    with torch.no_grad():
        assert torch.equal(probs, m(x))
    assert bool(torch.isfinite(out).all())


def test_data_parallel_trainer_runs_the_weighted_loss_on_a_logits_network():
    """world size 1, deterministic, the atomics-summed biases (LOOSE) frozen: two weighted trainer steps == by hand, to the bit"""
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp, ops
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    x, td, kw = _small_data(3, 7)
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
                    m.forward_backward(x, td, 1.0, 0.3, **kw)
                    opt.step()
            else:
                tr = ddp.DataParallelTrainer(m, lr=0.01, momentum=0.9, w_dice=0.3, class_weight=kw["class_weight"].tolist(),
                                             ignore_index=kw["ignore_index"])
                assert torch.equal(tr.class_weight, kw["class_weight"])       # the sequence was converted once
                for _ in range(2):
                    tr.step(x, td, pixel_weight=kw["pixel_weight"])
            res.append({k: p.detach().clone() for k, p in m.named_parameters()})
    finally:
        e.deterministic = keep
    bad = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
    assert bad == [], bad
    moved = _sd_net("AttU_Net", "f32", dict(channels=[16, 32, 64, 128, 256]), seed=12)
    assert not torch.equal(moved.Conv1.init_conv.weight.cuda(), res[0]["Conv1.init_conv.weight"])


def test_data_parallel_trainer_runs_the_weighted_loss_on_unet():
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD
    x, td, kw = _small_data(4, 8)
    m = _small_unet()
    tr = ddp.DataParallelTrainer(m, lr=0.05, momentum=0.9, class_weight=kw["class_weight"], ignore_index=kw["ignore_index"])
    for _ in range(2):
        loss = tr.step(x, td, pixel_weight=kw["pixel_weight"])
    got = tr.opt.flat_p.cpu().numpy()
    assert bool(torch.isfinite(loss).all())
    m2 = _small_unet()
    opt = FusedSGD(list(m2.named_parameters()), lr=0.05, momentum=0.9)
    for _ in range(2):
        m2.forward_backward(x, td, **kw)
        opt.step()
    ref = opt.flat_p.cpu().numpy()
    # weight gradients are summed with fp32 atomics (order varies run to run): fp32 round-off, not bit equality
    err = np.abs(got - ref).max()
    print(f"flat parameters: max err {err:.3e}, max |ref| {np.abs(ref).max():.3e}")
    assert err <= 3e-4 * np.abs(ref).max()
    assert not np.array_equal(ref, FusedSGD(list(_small_unet().named_parameters()), lr=0.05).flat_p.cpu().numpy())
    # the weighted loss is not captured in a graph: refused, at construction for the constants and in step() for the map
    with pytest.raises(NotImplementedError, match="use_graph=True captures the unweighted fused step only"):
        ddp.DataParallelTrainer(_small_unet(), use_graph=True, ignore_index=255)
    trg = ddp.DataParallelTrainer(_small_unet(), use_graph=True)
    with pytest.raises(NotImplementedError, match="pixel_weight map needs use_graph=False"):
        trg.step(x, td.clamp(0, 3), pixel_weight=kw["pixel_weight"])


def test_full_size_cfg4_attunet_bf16_weighted():
    """cfg4 AttU_Net(1, 3) at 2 x 496 x 768, production dtype, all three options: finite, and torch's weighted loss"""
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net.unet import AttU_Net
    torch.manual_seed(0)
    m = AttU_Net(1, 3).cuda().train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 1, 496, 768, generator=g).cuda()
    td, cw, pw = _options_for(torch.randint(0, 3, (2, 496, 768), generator=g), 3, 33, 255)
    out = m.forward_backward(x, td, class_weight=cw, pixel_weight=pw, ignore_index=255)
    assert torch.isfinite(out).all()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    with torch.no_grad():
        ref = float(_torch_weighted(m(x), td, cw, pw, 255))
    print(f"loss {float(out[0]):.6f} torch {ref:.6f}")
    assert abs(float(out[0]) - ref) <= 3e-2 * max(1.0, abs(ref)), (float(out[0]), ref)
