"""CPU: the binary / multi-label loss head (sigmoid BCE + soft Dice) -- tests/bce_ref.py against float64 torch autograd, the
host-side argument checks of the oct_bce_loss_* entry points (every call below fails before a launch), and the Python-side
refusals, none of which needs a device.  tests/test_gpu_bce_loss.py holds the kernels to bce_ref."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bce_ref as R


def torch_reference(x, t, w_bce, w_dice, eps=1e-7, pos_weight=None, pixel_weight=None, ignore_value=None):
    """The definition in torch.float64, differentiated by autograd: ([loss, bce, dice], d(loss)/dx)"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(True)
    tt = torch.from_numpy(np.ascontiguousarray(t)).reshape(xt.shape)
    c = xt.shape[1]
    valid = torch.ones_like(tt, dtype=torch.bool) if ignore_value is None else tt != ignore_value
    tf = torch.where(valid, tt, torch.zeros_like(tt)).double()
    pw = None if pos_weight is None else torch.as_tensor(np.asarray(pos_weight), dtype=torch.float64).reshape(1, c, 1, 1)
    per = F.binary_cross_entropy_with_logits(xt, tf, pos_weight=pw, reduction="none")
    omega = valid.double()
    if pixel_weight is not None:
        omega = omega * torch.as_tensor(np.asarray(pixel_weight), dtype=torch.float64)[:, None]
    bce = (omega * per).sum() / omega.sum()
    s, v = torch.sigmoid(xt), valid.double()
    inter, ps, ys = (s * tf * v).sum((0, 2, 3)), (s * v).sum((0, 2, 3)), (tf * v).sum((0, 2, 3))
    dice = 1.0 - ((2.0 * inter + eps) / (ps + ys + eps)).mean() if w_dice != 0.0 else torch.zeros((), dtype=torch.float64)
    loss = w_bce * bce + w_dice * dice
    loss.backward()
    return np.array([loss.item(), bce.item(), dice.item()]), xt.grad.numpy()


def binary_case(classes, seed=5, shape=(2, 9, 11), ignore_value=None, ignored=()):
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    x = (3.0 * torch.randn(n, classes, h, w, generator=g)).double().numpy()
    t = (torch.rand(n, classes, h, w, generator=g) < 0.4).to(torch.uint8).numpy()
    pos = (0.25 + 3.75 * torch.rand(classes, generator=g)).double().numpy()
    pm = (1.0 + 9.0 * (torch.rand(n, h, w, generator=g) < 0.1).double()).numpy()
    for idx in ignored:
        t[idx] = ignore_value
    return x, t, pos, pm


# ---- 1. the reference against float64 autograd ---------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [1, 3])
@pytest.mark.parametrize("w_dice", [0.0, 0.7])
@pytest.mark.parametrize("options", [False, True])
def test_reference_is_torch_autograd_in_float64(classes, w_dice, options):
    ign = ((0, 0, 1, 2), (1, classes - 1, 8, 10)) if options else ()
    x, t, pos, pm = binary_case(classes, ignore_value=255, ignored=ign)
    kw = dict(pos_weight=pos, pixel_weight=pm, ignore_value=255) if options else {}
    ref, rdl = R.loss_and_grad(x, t, 0.8, w_dice, **kw)
    want, wdl = torch_reference(x, t, 0.8, w_dice, **kw)
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=0)
    assert np.abs(rdl - wdl).max() <= 1e-12 * np.abs(wdl).max()
    if w_dice == 0.0:
        assert ref[2] == 0.0 and ref[0] == 0.8 * ref[1]
    for idx in ign:
        assert rdl[idx] == 0.0


def test_reference_without_options_is_f_binary_cross_entropy_with_logits():
    x, t, _, _ = binary_case(3)
    ref, rdl = R.loss_and_grad(x, t)
    xt = torch.from_numpy(x).requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(xt, torch.from_numpy(t).double())
    want.backward()
    assert abs(ref[0] - want.item()) <= 1e-12 * want.item()
    assert np.abs(rdl - xt.grad.numpy()).max() <= 1e-12 * np.abs(rdl).max()
    # a (B, H, W) target for one channel; an upstream gradient scales dx
    x1, t1, _, _ = binary_case(1)
    np.testing.assert_array_equal(R.loss_and_grad(x1, t1[:, 0], 1.0, 0.5)[1], R.loss_and_grad(x1, t1, 1.0, 0.5)[1])
    np.testing.assert_allclose(R.loss_and_grad(x, t, 1.0, 0.5, g=0.25)[1], 0.25 * R.loss_and_grad(x, t, 1.0, 0.5)[1], rtol=1e-15)


def test_reference_edge_cases():
    x, t, pos, pm = binary_case(2, ignore_value=255, ignored=((0, 1, 0, 0), (1, 0, 3, 3)))
    base, bdl = R.loss_and_grad(x, t, 1.0, 0.5, pos_weight=pos, pixel_weight=pm, ignore_value=255)
    for bad in (np.nan, np.inf, -np.inf):           # a logit under an ignored element cannot leak
        x2 = x.copy()
        x2[0, 1, 0, 0] = x2[1, 0, 3, 3] = bad
        out, dl = R.loss_and_grad(x2, t, 1.0, 0.5, pos_weight=pos, pixel_weight=pm, ignore_value=255)
        np.testing.assert_array_equal(out, base)
        np.testing.assert_array_equal(dl, bdl)
    assert np.isnan(R.forward(x, np.full_like(t, 255), ignore_value=255)[0][0])      # everything ignored
    t7 = t.copy()
    t7[0, 0, 2, 2] = 7
    assert np.isnan(R.forward(x, t7, ignore_value=255)[0][0])                         # a valid label of 7
    # the mask: >= tau, a NaN logit gives 0, tau is 0 at 0.5
    assert R.threshold_to_tau(0.5) == 0.0 and R.threshold_to_tau(0.3) == float(np.float32(np.log(0.3 / 0.7)))
    xs = np.array([[[[0.0, -0.0, np.nan, 1.0, -1.0]]]], dtype=np.float32)
    np.testing.assert_array_equal(R.mask(xs, 0.0), [[[[1, 1, 0, 1, 0]]]])


# ---- 2. the C ABI refuses bad arguments before a launch -----------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


FAKE = 0x1000    # never dereferenced: every call below is one that validation refuses, so nothing is ever launched

NAMES = ("oct_bce_loss_weight_sum", "oct_bce_loss_forward", "oct_bce_loss_backward")


def _call(L, name, d, layout=0, logits=FAKE, target=FAKE, out=FAKE, wsum=FAKE, rows=FAKE, coef=None, ignore=(0, 0), pm=None):
    """ONE entry point with arguments that must be refused: asserts the -22 and returns the message.  Only refused calls may
    be made here: on a machine with a GPU an accepted one would launch a kernel on these pointers."""
    lib = L.lib()
    dp = C.byref(d) if d is not None else None
    has, ig = ignore
    if name == "oct_bce_loss_weight_sum":
        rc = lib.oct_bce_loss_weight_sum(dp, target, pm, has, ig, rows, wsum, None)
    elif name == "oct_bce_loss_forward":
        rc = lib.oct_bce_loss_forward(dp, layout, logits, target, None, pm, has, ig, 1, 0.0, None, rows, None)
    else:
        rc = lib.oct_bce_loss_backward(dp, layout, logits, target, None, pm, has, ig, wsum, coef, 1.0, None, out,
                                       rows if coef is None else FAKE, None)
    msg = L.last_error()
    assert rc == -22, (name, rc, msg)
    return msg


def test_new_exports_are_bound_and_the_version_stays(L):
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
    assert L.lib().oct_version() == 220


@pytest.mark.parametrize("classes", [0, 17])
def test_channels_out_of_range_are_refused(L, classes):
    d = L.HeadDesc(L.DT_F32, 2, 8, 8, 1, classes)
    for name in NAMES:
        assert f"{name}: classes {classes} not in [1,16]" in _call(L, name, d)


def test_null_pointers_and_bad_ignore_values_are_refused(L):
    d = L.HeadDesc(L.DT_BF16, 2, 8, 8, 1, 3)
    fwd, bwd, wsum = "oct_bce_loss_forward", "oct_bce_loss_backward", "oct_bce_loss_weight_sum"
    for name in NAMES:
        assert f"{name}: null descriptor" in _call(L, name, None)
    for name in (fwd, bwd):
        assert f"{name}: null pointer (logits" in _call(L, name, d, logits=None)
    for name in NAMES:
        msg = _call(L, name, d, target=None, ignore=(1, 255))
        assert f"{name}: null pointer" in msg and "target" in msg
    for name in (wsum, fwd):                   # the backward's rows are optional
        assert f"{name}: null pointer" in _call(L, name, d, rows=None)
    for name in (wsum, bwd):
        assert "wsum" in _call(L, name, d, wsum=None, ignore=(1, 255))
    assert "needs wsum" in _call(L, bwd, d, wsum=None, pm=FAKE)
    assert f"{bwd}: null pointer" in _call(L, bwd, d, out=None)
    assert "without a Dice term" in _call(L, bwd, d, coef=FAKE)
    for bad in (0, 1, 256, -1):
        for name in NAMES:
            assert f"{name}: ignore_value {bad} not in [2,255]" in _call(L, name, d, ignore=(1, bad))
    assert L.lib().oct_bce_loss_forward(C.byref(d), L.SEG_NHWC, FAKE, None, None, None, 0, 0, 0, 0.0, None, None, None) == -22
    assert "neither mask nor loss_partials" in L.last_error()


def test_bad_layout_dtype_and_shape_are_refused(L):
    d = L.HeadDesc(L.DT_F32, 2, 8, 8, 1, 3)
    for layout in (2, -1):
        for name in NAMES[1:]:                 # the weight sum takes no layout
            assert f"{name}: bad layout {layout}" in _call(L, name, d, layout)
    for name in NAMES[1:]:
        assert f"{name}: NCHW logits are fp32 only" in _call(L, name, L.HeadDesc(L.DT_BF16, 2, 8, 8, 1, 3), L.SEG_NCHW)
    for name in NAMES:
        assert f"{name}: bad dtype 7" in _call(L, name, L.HeadDesc(7, 2, 8, 8, 1, 3))
        assert f"{name}: bad shape" in _call(L, name, L.HeadDesc(L.DT_F32, 2, 0, 8, 1, 3))


# ---- 3. Python-side refusals, before a launch ---------------------------------------------------------------------------
def test_options_are_checked_before_anything_runs():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import _binary_options
    dev = torch.device("cuda", 0)        # only compared: nothing below touches a device
    geo = (2, 8, 12, 3, dev)
    assert _binary_options(None, None, None, *geo) is None
    with pytest.raises(RuntimeError, match="pos_weight must have 3 entries"):
        _binary_options([1.0, 2.0], None, None, *geo)
    with pytest.raises(RuntimeError, match="pos_weight must have 3 entries"):
        _binary_options(torch.ones(4), None, None, *geo)
    with pytest.raises(RuntimeError, match="pos_weight must be fp32"):
        _binary_options(torch.ones(3, dtype=torch.float64), None, None, *geo)
    with pytest.raises(RuntimeError, match="pos_weight is on cpu"):
        _binary_options(torch.ones(3), None, None, *geo)
    with pytest.raises(RuntimeError, match=r"pixel_weight must have shape \(2, 8, 12\)"):
        _binary_options(None, torch.ones(2, 3, 8, 12), None, *geo)
    with pytest.raises(RuntimeError, match="pixel_weight must be an fp32 tensor"):
        _binary_options(None, torch.ones(2, 8, 12, dtype=torch.float64), None, *geo)
    with pytest.raises(RuntimeError, match="pixel_weight is on cpu"):
        _binary_options(None, torch.ones(2, 8, 12), None, *geo)
    for bad in (2.0, "255", True, torch.tensor(3)):
        with pytest.raises(TypeError, match="ignore_value must be an int"):
            _binary_options(None, None, bad, *geo)
    for bad in (1, 256, 0, -1):
        with pytest.raises(ValueError, match=rf"ignore_value {bad} is not in \[2, 255\]"):
            _binary_options(None, None, bad, *geo)
    assert _binary_options(None, None, 2, *geo) == (None, None, 1, 2)
    cpu = (2, 8, 12, 3, torch.device("cpu"))
    pw, pm, has, ig = _binary_options([1.0, 2.0, 3.0], torch.ones(2, 8, 12), 255, *cpu)
    assert pw.dtype == torch.float32 and pw.tolist() == [1.0, 2.0, 3.0] and pm.shape == (2, 8, 12) and (has, ig) == (1, 255)


def test_target_dtype_and_shape_are_checked():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import _binary_target
    cpu = torch.device("cpu")
    for bad in (torch.zeros(2, 3, 8, 12, dtype=torch.int64), torch.zeros(2, 3, 8, 12), torch.zeros(2, 3, 8, 12, dtype=torch.int8)):
        with pytest.raises(RuntimeError, match=r"target must be uint8 or bool of shape \(2, 3, 8, 12\)"):
            _binary_target(bad, 2, 3, 8, 12, cpu)
    for shape in ((2, 8, 12), (2, 3, 12, 8), (2, 1, 8, 12), (3, 8, 12)):
        with pytest.raises(RuntimeError, match=r"target must be uint8 or bool of shape \(2, 3, 8, 12\)"):
            _binary_target(torch.zeros(shape, dtype=torch.uint8), 2, 3, 8, 12, cpu)
    with pytest.raises(RuntimeError, match="target is on cpu"):
        _binary_target(torch.zeros(2, 3, 8, 12, dtype=torch.uint8), 2, 3, 8, 12, torch.device("cuda", 0))
    # one channel takes (B, H, W); bool is viewed as uint8 without a copy
    assert _binary_target(torch.zeros(2, 8, 12, dtype=torch.uint8), 2, 1, 8, 12, cpu).shape == (2, 8, 12)
    b = torch.ones(2, 3, 8, 12, dtype=torch.bool)
    v = _binary_target(b, 2, 3, 8, 12, cpu)
    assert v.dtype == torch.uint8 and v.data_ptr() == b.data_ptr() and int(v.sum()) == b.numel()


def test_threshold_must_lie_inside_the_unit_interval():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import mask_threshold
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match=r"threshold must lie in \(0, 1\)"):
            mask_threshold(bad)
    assert mask_threshold(0.5) == 0.0
    assert mask_threshold(0.3) == R.threshold_to_tau(0.3) == float(np.float32(np.log(0.3 / 0.7)))


def test_functional_loss_refuses_cpu_tensors():
    from retinal_oct_image_segmentation_via_deep_learning_amd import OctError
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import binary_cross_entropy_dice
    x, t = torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4, dtype=torch.uint8)
    with pytest.raises(OctError, match="device tensor"):
        binary_cross_entropy_dice(x, t)
    with pytest.raises(OctError, match="device tensor"):
        binary_cross_entropy_dice(x, t, 1.0, 0.5, pos_weight=[1.0, 1.0, 1.0], ignore_value=255)


def _logits_nets():
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.ReLayNet_2017 import ReLayNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net import unet as U
    return {"AttU_Net": lambda c: U.AttU_Net(1, c, channels=[4, 8, 8, 8, 8]),
            "MGUNet_2": lambda c: M.MGUNet_2(1, c, feature_scale=16), "ReLayNet": lambda c: ReLayNet(1, c, num_filters=8)}


@pytest.mark.parametrize("name", ["AttU_Net", "MGUNet_2", "ReLayNet"])
def test_logits_networks_refuse_before_the_forward(name):
    m = _logits_nets()[name](2).train()
    x, t = torch.zeros(1, 1, 48, 48), torch.zeros(1, 2, 48, 48, dtype=torch.uint8)
    for call in (m.forward_backward_binary, m.loss_binary):
        with pytest.raises(RuntimeError, match="pos_weight must have 2 entries"):
            call(x, t, pos_weight=[1.0])
        with pytest.raises(RuntimeError, match="pixel_weight must have shape"):
            call(x, t, pixel_weight=torch.ones(1, 48, 47))
        with pytest.raises(ValueError, match=r"ignore_value 1 is not in \[2, 255\]"):
            call(x, t, ignore_value=1)
        with pytest.raises(ValueError, match=r"ignore_value 256 is not in \[2, 255\]"):
            call(x, t, ignore_value=256)
        with pytest.raises(RuntimeError, match="target must be uint8 or bool"):
            call(x, t.long())
        with pytest.raises(RuntimeError, match="target must be uint8 or bool"):
            call(x, t[:, 0])                       # (B, H, W) is for one channel only
    for thr in (0, 1):
        with pytest.raises(ValueError, match="threshold must lie in"):
            m.predict_mask(x, thr)
    with pytest.raises(RuntimeError, match="needs train"):
        m.eval().forward_backward_binary(x, t)
    assert all(p.grad is None for p in m.parameters())


def test_seventeen_channels_are_refused_with_the_existing_wording():
    m = _logits_nets()["AttU_Net"](17).train()
    x, t = torch.zeros(1, 1, 48, 48), torch.zeros(1, 17, 48, 48, dtype=torch.uint8)
    for call in (lambda: m.forward_backward_binary(x, t), lambda: m.loss_binary(x, t), lambda: m.predict_mask(x)):
        with pytest.raises(NotImplementedError, match=r"the HIP loss kernels take at most 16 classes \(got 17\)"):
            call()


def test_engine_networks_refuse_before_the_forward():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import BioUNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet3d import UNet3D
    x, t = torch.zeros(1, 1, 32, 32), torch.zeros(1, 32, 32, dtype=torch.uint8)
    for m in (UNet(1, 1, init_features=4).train(), BioUNet(1, 1).train()):
        for call in (m.forward_backward_binary, m.loss_binary):
            with pytest.raises(RuntimeError, match="pos_weight must have 1 entries"):
                call(x, t, pos_weight=torch.ones(5))
            with pytest.raises(RuntimeError, match="pixel_weight must have shape"):
                call(x, t, pixel_weight=torch.ones(32, 32))
            with pytest.raises(ValueError, match=r"ignore_value 1 is not in"):
                call(x, t, ignore_value=1)
            with pytest.raises(RuntimeError, match="target must be uint8 or bool"):
                call(x, t.float())
        for thr in (0, 1):
            with pytest.raises(ValueError, match="threshold must lie in"):
                m.predict_mask(x, thr)
        with pytest.raises(RuntimeError, match="needs train"):
            m.eval().forward_backward_binary(x, t)
        assert all(p.grad is None for p in m.parameters())
    # (an engine network with 17 channels cannot be built at all: UNetEngine refuses it)
    # the volumetric network says that it has no binary head
    v = UNet3D(1, 1, init_features=4).train()
    xv, tv = torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 16, 16, 16, dtype=torch.uint8)
    for call in (lambda: v.forward_backward_binary(xv, tv), lambda: v.loss_binary(xv, tv), lambda: v.predict_mask(xv)):
        with pytest.raises(NotImplementedError, match="2-D networks only"):
            call()


def test_trainer_refuses_the_binary_loss_under_a_graph():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet, ddp
    m = UNet(1, 1, init_features=4)
    with pytest.raises(NotImplementedError, match="loss='binary' needs use_graph=False"):
        ddp.DataParallelTrainer(m, loss="binary", use_graph=True)
    with pytest.raises(NotImplementedError, match="loss='binary' needs use_graph=False"):
        ddp.DataParallelTrainer(m, loss="binary", use_graph=True, pos_weight=[2.0], ignore_value=255)
    with pytest.raises(ValueError, match="one of 'ce', 'binary'"):
        ddp.DataParallelTrainer(m, loss="bce")
    with pytest.raises(ValueError, match="belong to loss='binary'"):
        ddp.DataParallelTrainer(m, pos_weight=[2.0])
    with pytest.raises(ValueError, match="belong to loss='ce'"):
        ddp.DataParallelTrainer(m, loss="binary", ignore_index=255)
    assert all(p.grad is None for p in m.parameters())     # refused before anything was re-homed
    sig = inspect.signature(ddp.DataParallelTrainer.__init__)
    assert sig.parameters["loss"].default == "ce"
    assert sig.parameters["pos_weight"].default is None and sig.parameters["ignore_value"].default is None


# ---- 4. the signatures the issue names -----------------------------------------------------------------------------------
def test_signatures():
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import SegLossMixin, binary_cross_entropy_dice
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import _EngineNet
    opts = [("pos_weight", None), ("pixel_weight", None), ("ignore_value", None)]
    head = [("w_bce", 1.0), ("w_dice", 0.0), ("dice_eps", 1e-7)]
    sig = [(p.name, p.default) for p in inspect.signature(binary_cross_entropy_dice).parameters.values()]
    assert sig[2:] == head + opts and [n for n, _ in sig[:2]] == ["logits", "target"]
    for owner in (_EngineNet, SegLossMixin):
        fb = [(p.name, p.default) for p in inspect.signature(owner.forward_backward_binary).parameters.values()]
        assert fb[3:] == head + [("stage_hook", None)] + opts and [n for n, _ in fb[:3]] == ["self", "x", "target"]
        lo = [(p.name, p.default) for p in inspect.signature(owner.loss_binary).parameters.values()]
        assert lo[3:] == head + opts
        pm = [(p.name, p.default) for p in inspect.signature(owner.predict_mask).parameters.values()]
        assert pm[1:] == [("x", inspect._empty), ("threshold", 0.5)]
