"""CPU: the weighted loss (class weights, pixel weight map, ignore_index) -- its float64 reference, the host-side argument
checks of the oct_seg_loss_*_weighted entry points (every call below fails before a launch), the Python-side refusals, and the
signatures that carry the three keywords.

The float64 reference lives here (`reference_loss`): the definition in torch.float64 on the CPU, differentiated by autograd.
  valid_i = (t_i != ignore_index),  omega_i = valid_i * class_weight[t_i] * pixel_weight[i]
  CE   = sum omega_i * (-log softmax[t_i]) / sum omega_i
  Dice = 1 - mean_c (2 I_c + eps) / (P_c + Y_c + eps) over the valid pixels, unweighted
  loss = w_ce CE + w_dice Dice
tests/test_gpu_seg_loss_weighted.py holds the kernels to it."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu


def reference_loss(x, t, w_ce=1.0, w_dice=0.0, eps=1e-7, class_weight=None, pixel_weight=None, ignore_index=None):
    """x: (B, C, H, W) float64 array, t: (B, H, W) int64 array -> ([loss, ce, dice], d(loss)/dx), float64"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(True)
    tt = torch.from_numpy(np.ascontiguousarray(t)).long()
    ncls = xt.shape[1]
    valid = torch.ones_like(tt, dtype=torch.bool) if ignore_index is None else tt != ignore_index
    ts = torch.where(valid, tt, torch.zeros_like(tt))            # a gatherable label where the pixel does not count
    logp = F.log_softmax(xt, 1)
    nll = -logp.gather(1, ts[:, None])[:, 0]
    omega = valid.double()
    if class_weight is not None:
        omega = omega * torch.as_tensor(np.asarray(class_weight), dtype=torch.float64)[ts]
    if pixel_weight is not None:
        omega = omega * torch.as_tensor(np.asarray(pixel_weight), dtype=torch.float64)
    ce = (omega * torch.where(valid, nll, torch.zeros_like(nll))).sum() / omega.sum()
    p = logp.exp()
    v = valid[:, None].double()
    onehot = F.one_hot(ts, ncls).permute(0, 3, 1, 2).double() * v
    inter, ps, ys = (p * onehot).sum((0, 2, 3)), (p * v).sum((0, 2, 3)), onehot.sum((0, 2, 3))
    dice = 1.0 - ((2.0 * inter + eps) / (ps + ys + eps)).mean()
    loss = w_ce * ce + w_dice * dice
    loss.backward()
    return np.array([loss.item(), ce.item(), dice.item()]), xt.grad.numpy()


def weighted_case(shape, classes, seed, ignore_index):
    """class weights uniform in [0.25, 4], map 1 + 9 [rand < 0.1], and the pixels to ignore: 20 % at random plus image 0"""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    cw = (0.25 + 3.75 * torch.rand(classes, generator=g)).float()
    pw = (1.0 + 9.0 * (torch.rand(n, h, w, generator=g) < 0.1).float())
    ign = torch.rand(n, h, w, generator=g) < 0.2
    ign[0] = True
    return cw.numpy(), pw.numpy(), ign.numpy()


def _inputs(shape=(3, 13, 17), classes=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(shape[0], classes, shape[1], shape[2], generator=g)
    t = torch.randint(0, classes, shape, generator=g)
    return x.double().numpy(), t.numpy()


# ---- 1. the reference itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
def test_reference_without_options_is_the_oracle(w_dice):
    x, t = _inputs()
    ref, rdl = reference_loss(x, t, 1.0, w_dice)
    loss, ce, dice, cache = ref_cpu.loss_head_fwd(x, t, 1.0, w_dice)
    np.testing.assert_allclose(ref, [loss, ce, dice], rtol=0, atol=1e-13)
    assert np.abs(rdl - ref_cpu.loss_head_bwd(cache, 1.0, w_dice)).max() <= 1e-15


@pytest.mark.parametrize("ignore_index", [-100, 255])
def test_reference_is_f_cross_entropy_with_weights_and_ignored_pixels(ignore_index):
    x, t = _inputs()
    cw, pw, ign = weighted_case(t.shape, 5, 11, ignore_index)
    t = np.where(ign, ignore_index, t)
    ref, rdl = reference_loss(x, t, class_weight=cw, ignore_index=ignore_index)
    xt = torch.from_numpy(x).requires_grad_(True)
    tt, cwt = torch.from_numpy(t), torch.from_numpy(cw).double()
    want = F.cross_entropy(xt, tt, weight=cwt, ignore_index=ignore_index)
    want.backward()
    assert abs(ref[0] - want.item()) <= 1e-13 and ref[0] == ref[1]
    assert np.abs(rdl - xt.grad.numpy()).max() <= 1e-15
    assert (rdl[0] == 0).all() and (rdl.transpose(0, 2, 3, 1)[ign] == 0).all()       # ignored: exactly 0
    # with a map: (per-pixel weighted CE * map).sum() / sum omega
    ref, rdl = reference_loss(x, t, class_weight=cw, pixel_weight=pw, ignore_index=ignore_index)
    xt = torch.from_numpy(x).requires_grad_(True)
    pwt = torch.from_numpy(pw).double()
    per = F.cross_entropy(xt, tt, weight=cwt, ignore_index=ignore_index, reduction="none")
    omega = (tt != ignore_index).double() * cwt[torch.where(tt != ignore_index, tt, 0)] * pwt
    want = (per * pwt).sum() / omega.sum()
    want.backward()
    assert abs(ref[0] - want.item()) <= 1e-13
    assert np.abs(rdl - xt.grad.numpy()).max() <= 1e-15


# ---- 2. the C ABI refuses bad arguments before a launch -----------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


FAKE = 0x1000    # never dereferenced: validation fails first


def _calls(L, d, layout, logits=FAKE, target=FAKE, out=FAKE, wsum=FAKE, rows=FAKE, coef=None):
    """the four new entry points with one descriptor; (name, return code, message) each"""
    lib = L.lib()
    dp = C.byref(d) if d is not None else None
    res = []
    for name, rc in (
            ("oct_seg_loss_weight_sum", lambda: lib.oct_seg_loss_weight_sum(dp, target, None, None, 1, -100, rows, wsum, None)),
            ("oct_seg_loss_forward_weighted",
             lambda: lib.oct_seg_loss_forward_weighted(dp, layout, logits, target, None, None, 1, -100, rows, None)),
            ("oct_seg_loss_backward_weighted",
             lambda: lib.oct_seg_loss_backward_weighted(dp, layout, logits, target, None, None, 0, 0, wsum, coef, 1.0, None, out,
                                                        rows if coef is None else FAKE, None)),
            ("oct_seg_loss_finalize_weighted",
             lambda: lib.oct_seg_loss_finalize_weighted(dp, rows, 4, 1.0, 0.0, 1e-7, out, out, None, None))):
        res.append((name, rc(), L.last_error()))
    return res


def test_new_exports_are_bound(L):
    for name in ("oct_seg_loss_weight_sum", "oct_seg_loss_forward_weighted", "oct_seg_loss_backward_weighted",
                 "oct_seg_loss_finalize_weighted"):
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
    assert L.lib().oct_version() == 220


@pytest.mark.parametrize("classes", [0, 17])
def test_weighted_classes_out_of_range_are_refused(L, classes):
    d = L.HeadDesc(L.DT_F32, 2, 8, 8, 1, classes)
    for name, rc, msg in _calls(L, d, L.SEG_NHWC):
        assert rc == -22 and f"{name}: classes {classes} not in [1,16]" in msg, (name, rc, msg)


def test_weighted_null_pointers_are_refused(L):
    d = L.HeadDesc(L.DT_BF16, 2, 8, 8, 1, 3)
    for name, rc, msg in _calls(L, None, L.SEG_NHWC):
        assert rc == -22 and f"{name}: null descriptor" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, d, L.SEG_NHWC, logits=None):
        if "forward" in name or "backward" in name:
            assert rc == -22 and f"{name}: null pointer (logits)" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, d, L.SEG_NHWC, target=None):
        if "finalize" not in name:
            assert rc == -22 and f"{name}: null pointer (target" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, d, L.SEG_NHWC, rows=None):
        if "backward" not in name:       # the backward's rows are optional
            assert rc == -22 and f"{name}: null pointer" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, d, L.SEG_NHWC, wsum=None):
        if name in ("oct_seg_loss_weight_sum", "oct_seg_loss_backward_weighted"):
            assert rc == -22 and "wsum" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, d, L.SEG_NHWC, out=None):
        if name in ("oct_seg_loss_backward_weighted", "oct_seg_loss_finalize_weighted"):
            assert rc == -22 and f"{name}: null pointer" in msg, (name, rc, msg)
    name, rc, msg = _calls(L, d, L.SEG_NHWC, coef=FAKE)[2]
    assert rc == -22 and "without a Dice term" in msg
    assert L.lib().oct_seg_loss_finalize_weighted(C.byref(d), FAKE, 0, 1.0, 0.0, 1e-7, FAKE, FAKE, None, None) == -22
    assert "bad row count 0" in L.last_error()


def test_weighted_bad_layout_dtype_and_shape_are_refused(L):
    d = L.HeadDesc(L.DT_F32, 2, 8, 8, 1, 3)
    for layout in (2, -1):
        for name, rc, msg in _calls(L, d, layout):
            if "forward" in name or "backward" in name:
                assert rc == -22 and f"{name}: bad layout {layout}" in msg, (name, rc, msg)
    d = L.HeadDesc(L.DT_BF16, 2, 8, 8, 1, 3)
    for name, rc, msg in _calls(L, d, L.SEG_NCHW):
        if "forward" in name or "backward" in name:
            assert rc == -22 and f"{name}: NCHW logits are fp32 only" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, L.HeadDesc(7, 2, 8, 8, 1, 3), L.SEG_NHWC):
        assert rc == -22 and f"{name}: bad dtype 7" in msg, (name, rc, msg)
    for name, rc, msg in _calls(L, L.HeadDesc(L.DT_F32, 2, 0, 8, 1, 3), L.SEG_NHWC):
        assert rc == -22 and f"{name}: bad shape" in msg, (name, rc, msg)


# ---- 3. Python-side refusals, before a launch ---------------------------------------------------------------------------
def test_options_are_checked_before_anything_runs():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import _options
    dev = torch.device("cuda", 0)        # only compared: nothing below touches a device
    geo = (2, 8, 12, 3, dev)
    assert _options(None, None, None, *geo) is None
    with pytest.raises(RuntimeError, match="class_weight must have 3 entries"):
        _options([1.0, 2.0], None, None, *geo)
    with pytest.raises(RuntimeError, match="class_weight must have 3 entries"):
        _options(torch.ones(4), None, None, *geo)
    with pytest.raises(RuntimeError, match="class_weight must be fp32"):
        _options(torch.ones(3, dtype=torch.float64), None, None, *geo)
    with pytest.raises(RuntimeError, match="class_weight is on cpu"):
        _options(torch.ones(3), None, None, *geo)
    with pytest.raises(RuntimeError, match=r"pixel_weight must have shape \(2, 8, 12\)"):
        _options(None, torch.ones(2, 12, 8), None, *geo)
    with pytest.raises(RuntimeError, match=r"pixel_weight must have shape"):
        _options(None, torch.ones(2, 1, 8, 12), None, *geo)
    with pytest.raises(RuntimeError, match="pixel_weight must be an fp32 tensor"):
        _options(None, torch.ones(2, 8, 12, dtype=torch.bfloat16), None, *geo)
    with pytest.raises(RuntimeError, match="pixel_weight must be an fp32 tensor"):
        _options(None, [[1.0]], None, *geo)
    with pytest.raises(RuntimeError, match="pixel_weight is on cpu"):
        _options(None, torch.ones(2, 8, 12), None, *geo)
    for bad in (1.0, "255", True, torch.tensor(3)):
        with pytest.raises(TypeError, match="ignore_index must be an int"):
            _options(None, None, bad, *geo)
    with pytest.raises(ValueError, match="not an int64"):
        _options(None, None, 2 ** 63, *geo)
    # ignore_index alone needs no tensor: the flag and the value the kernels get
    assert _options(None, None, -100, *geo) == (None, None, 1, -100)
    assert _options(None, None, 0, *geo) == (None, None, 1, 0)
    cpu = (2, 8, 12, 3, torch.device("cpu"))
    cw, pw, has, ig = _options([1.0, 2.0, 3.0], torch.ones(2, 8, 12), 255, *cpu)
    assert cw.dtype == torch.float32 and cw.tolist() == [1.0, 2.0, 3.0] and pw.shape == (2, 8, 12) and (has, ig) == (1, 255)


def _nets():
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.ReLayNet_2017 import ReLayNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net import unet as U
    return {"U_Net": lambda c: U.U_Net(1, c, channels=[64, 8, 8, 8, 8]),
            "AttU_Net": lambda c: U.AttU_Net(1, c, channels=[4, 8, 8, 8, 8]),
            "AttU_Net4": lambda c: U.AttU_Net4(1, c, channels=[4, 8, 8, 8]),
            "MGUNet": lambda c: M.MGUNet(1, c, feature_scale=16), "MGUNet_2": lambda c: M.MGUNet_2(1, c, feature_scale=16),
            "ReLayNet": lambda c: ReLayNet(1, c, num_filters=8)}


def test_functional_loss_refuses_cpu_tensors_and_bad_options():
    from retinal_oct_image_segmentation_via_deep_learning_amd import OctError
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    x, t = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(OctError, match="device tensor"):
        cross_entropy_dice(x, t, class_weight=[1.0, 1.0, 1.0], ignore_index=-100)
    with pytest.raises(OctError, match="device tensor"):
        cross_entropy_dice(x, t, pixel_weight=torch.ones(1, 4, 4))


@pytest.mark.parametrize("name", ["AttU_Net", "MGUNet_2", "ReLayNet"])
def test_networks_refuse_bad_options_before_the_forward(name):
    m = _nets()[name](3).train()
    x, t = torch.zeros(1, 1, 48, 48), torch.zeros(1, 48, 48, dtype=torch.int64)
    for call in (m.forward_backward, m.loss):
        with pytest.raises(RuntimeError, match="class_weight must have 3 entries"):
            call(x, t, class_weight=[1.0, 1.0])
        with pytest.raises(RuntimeError, match="pixel_weight must have shape"):
            call(x, t, pixel_weight=torch.ones(1, 48, 47))
        with pytest.raises(RuntimeError, match="pixel_weight must be an fp32 tensor"):
            call(x, t, pixel_weight=torch.ones(1, 48, 48, dtype=torch.float64))
        with pytest.raises(TypeError, match="ignore_index must be an int"):
            call(x, t, ignore_index=255.0)
    with pytest.raises(RuntimeError, match="needs train"):
        m.eval().forward_backward(x, t, ignore_index=255)
    assert all(p.grad is None for p in m.parameters())


def test_engine_networks_refuse_bad_options_before_the_forward():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import BioUNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet3d import UNet3D
    x, t = torch.zeros(1, 1, 32, 32), torch.zeros(1, 32, 32, dtype=torch.int64)
    for m in (UNet(1, 3, init_features=4).train(), BioUNet(1, 3).train()):
        for call in (m.forward_backward, m.loss):
            with pytest.raises(RuntimeError, match="class_weight must have 3 entries"):
                call(x, t, class_weight=torch.ones(5))
            with pytest.raises(RuntimeError, match="pixel_weight must have shape"):
                call(x, t, pixel_weight=torch.ones(32, 32))
            with pytest.raises(TypeError, match="ignore_index must be an int"):
                call(x, t, ignore_index=1.5)
        with pytest.raises(RuntimeError, match="needs train"):
            m.eval().forward_backward(x, t, ignore_index=255)
        assert all(p.grad is None for p in m.parameters())
    # the volumetric network says that it has no weighted loss
    v = UNet3D(1, 2, init_features=4).train()
    xv, tv = torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 16, 16, 16, dtype=torch.int64)
    for kw in (dict(class_weight=[1.0, 2.0]), dict(pixel_weight=torch.ones(1, 16, 16)), dict(ignore_index=255)):
        for call in (v.forward_backward, v.loss):
            with pytest.raises(NotImplementedError, match="2-D networks only"):
                call(xv, tv, **kw)


def test_trainer_refuses_the_weighted_loss_under_a_graph():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet, ddp
    m = UNet(1, 3, init_features=4)
    for kw in (dict(class_weight=[1.0, 2.0, 3.0]), dict(ignore_index=255)):
        with pytest.raises(NotImplementedError, match="use_graph=True captures the unweighted fused step only"):
            ddp.DataParallelTrainer(m, use_graph=True, **kw)
    assert all(p.grad is None for p in m.parameters())     # refused before anything was re-homed
    sig = inspect.signature(ddp.DataParallelTrainer.__init__)
    assert list(sig.parameters)[-2:] == ["class_weight", "ignore_index"]
    assert sig.parameters["class_weight"].default is None and sig.parameters["ignore_index"].default is None
    sig = inspect.signature(ddp.DataParallelTrainer.step)
    assert list(sig.parameters) == ["self", "x", "target", "pixel_weight"] and sig.parameters["pixel_weight"].default is None


# ---- 4. the keywords, everywhere the same ---------------------------------------------------------------------------------
NEW = [("class_weight", None), ("pixel_weight", None), ("ignore_index", None)]


def _tail(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][-3:]


def test_keywords_on_the_engine_networks_and_the_functional_loss():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import SegLossMixin, cross_entropy_dice
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import _EngineNet
    for owner in (_EngineNet, SegLossMixin):
        assert _tail(owner.forward_backward) == NEW and _tail(owner.loss) == NEW
        names = list(inspect.signature(owner.forward_backward).parameters)
        assert names.index("class_weight") == names.index("stage_hook") + 1
        assert "class_weight" not in inspect.signature(owner.predict).parameters
    assert _tail(cross_entropy_dice) == NEW
    assert list(inspect.signature(cross_entropy_dice).parameters)[:5] == ["logits", "target", "w_ce", "w_dice", "dice_eps"]


@pytest.mark.parametrize("name", ["U_Net", "AttU_Net", "AttU_Net4", "MGUNet", "MGUNet_2", "ReLayNet"])
def test_keywords_on_the_logits_networks(name):
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import _EngineNet
    m = _nets()[name](3)
    for fn in ("forward_backward", "loss"):
        got = [(p.name, p.default) for p in inspect.signature(getattr(m, fn)).parameters.values()]
        want = [(p.name, p.default) for p in list(inspect.signature(getattr(_EngineNet, fn)).parameters.values())[1:]
                if p.name != "want_probs"]
        assert got == want and got[-3:] == NEW, fn
