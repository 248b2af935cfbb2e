"""CPU: the oct_seg_loss_* entry points validate their arguments on the host (no GPU is touched: every call below fails
before a launch), and the logits networks' training extras refuse what they cannot do before they run anything."""
import ctypes as C
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


FAKE = 0x1000    # never dereferenced: validation fails first


def test_block_count_query(L):
    lib = L.lib()
    assert lib.oct_seg_loss_blocks(1, 3) == 1
    assert lib.oct_seg_loss_blocks(256, 3) == 1 and lib.oct_seg_loss_blocks(257, 3) == 2
    assert lib.oct_seg_loss_blocks(3 * 37 * 53, 16) == (3 * 37 * 53 + 255) // 256
    assert lib.oct_seg_loss_blocks(4 * 496 * 768, 3) == 1024     # grid-stride range: capped
    assert lib.oct_seg_loss_blocks(0, 3) == 0
    assert lib.oct_seg_loss_blocks(100, 0) == 0 and lib.oct_seg_loss_blocks(100, 17) == 0


@pytest.mark.parametrize("classes", [0, 17])
def test_classes_out_of_range_are_refused(L, classes):
    lib = L.lib()
    d = L.HeadDesc(L.DT_F32, 2, 8, 8, 1, classes)
    rc = lib.oct_seg_loss_forward(C.byref(d), L.SEG_NHWC, FAKE, FAKE, None, FAKE, None)
    assert rc == -22 and f"classes {classes} not in [1,16]" in L.last_error()
    rc = lib.oct_seg_loss_backward(C.byref(d), L.SEG_NCHW, FAKE, FAKE, None, 1.0, None, FAKE, None, None)
    assert rc == -22 and f"classes {classes} not in [1,16]" in L.last_error()


def test_null_pointers_are_refused(L):
    lib = L.lib()
    d = L.HeadDesc(L.DT_BF16, 2, 8, 8, 1, 3)
    assert lib.oct_seg_loss_forward(None, L.SEG_NHWC, FAKE, FAKE, None, FAKE, None) == -22
    assert "null descriptor" in L.last_error()
    assert lib.oct_seg_loss_forward(C.byref(d), L.SEG_NHWC, None, FAKE, None, FAKE, None) == -22
    assert "null pointer (logits)" in L.last_error()
    assert lib.oct_seg_loss_forward(C.byref(d), L.SEG_NHWC, FAKE, FAKE, None, None, None) == -22
    assert "neither argmax nor loss_partials" in L.last_error()
    assert lib.oct_seg_loss_forward(C.byref(d), L.SEG_NHWC, FAKE, None, None, FAKE, None) == -22
    assert "loss partials need a target" in L.last_error()
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        lg, tg, dl = args
        assert lib.oct_seg_loss_backward(C.byref(d), L.SEG_NHWC, lg, tg, None, 1.0, None, dl, None, None) == -22
        assert "null pointer" in L.last_error()
    assert lib.oct_seg_loss_backward(C.byref(d), L.SEG_NHWC, FAKE, FAKE, FAKE, 1.0, None, FAKE, FAKE, None) == -22
    assert "without a Dice term" in L.last_error()


def test_bad_layout_and_dtype_are_refused(L):
    lib = L.lib()
    d = L.HeadDesc(L.DT_F32, 2, 8, 8, 1, 3)
    for layout in (2, -1):
        assert lib.oct_seg_loss_forward(C.byref(d), layout, FAKE, FAKE, None, FAKE, None) == -22
        assert f"bad layout {layout}" in L.last_error()
        assert lib.oct_seg_loss_backward(C.byref(d), layout, FAKE, FAKE, None, 1.0, None, FAKE, None, None) == -22
        assert f"bad layout {layout}" in L.last_error()
    d = L.HeadDesc(L.DT_BF16, 2, 8, 8, 1, 3)
    assert lib.oct_seg_loss_forward(C.byref(d), L.SEG_NCHW, FAKE, FAKE, None, FAKE, None) == -22
    assert "NCHW logits are fp32 only" in L.last_error()
    d = L.HeadDesc(7, 2, 8, 8, 1, 3)
    assert lib.oct_seg_loss_forward(C.byref(d), L.SEG_NHWC, FAKE, FAKE, None, FAKE, None) == -22
    assert "bad dtype 7" in L.last_error()
    d = L.HeadDesc(L.DT_F32, 2, 0, 8, 1, 3)
    assert lib.oct_seg_loss_forward(C.byref(d), L.SEG_NHWC, FAKE, FAKE, None, FAKE, None) == -22
    assert "bad shape" in L.last_error()


def _nets():
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.ReLayNet_2017 import ReLayNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net import unet as U
    return {"U_Net": lambda c: U.U_Net(1, c, channels=[64, 8, 8, 8, 8]),
            "AttU_Net": lambda c: U.AttU_Net(1, c, channels=[4, 8, 8, 8, 8]),
            "AttU_Net4": lambda c: U.AttU_Net4(1, c, channels=[4, 8, 8, 8]),
            "MGUNet": lambda c: M.MGUNet(1, c, feature_scale=16), "MGUNet_2": lambda c: M.MGUNet_2(1, c, feature_scale=16),
            "ReLayNet": lambda c: ReLayNet(1, c, num_filters=8)}


@pytest.mark.parametrize("name", ["U_Net", "AttU_Net", "AttU_Net4", "MGUNet", "MGUNet_2", "ReLayNet"])
def test_logits_networks_have_the_engine_extras(name):
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import _EngineNet
    m = _nets()[name](3)
    for fn in ("forward_backward", "loss", "predict"):
        got = inspect.signature(getattr(m, fn))
        want = inspect.signature(getattr(_EngineNet, fn))
        params = [(p.name, p.default) for p in list(want.parameters.values())[1:] if p.name != "want_probs"]
        assert [(p.name, p.default) for p in got.parameters.values()] == params, fn
    x, t = torch.zeros(1, 1, 48, 48), torch.zeros(1, 48, 48, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="needs train"):
        m.eval().forward_backward(x, t)
    big = _nets()[name](17).train()
    for call in (lambda: big.forward_backward(x, t), lambda: big.loss(x, t), lambda: big.predict(x)):
        with pytest.raises(NotImplementedError, match="at most 16 classes"):
            call()


def test_data_parallel_trainer_refuses_graphs_for_autograd_networks():
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp
    m = _nets()["AttU_Net"](3)
    with pytest.raises(NotImplementedError, match="use_graph"):
        ddp.DataParallelTrainer(m, use_graph=True)
    assert all(p.grad is None for p in m.parameters())     # refused before anything was re-homed


def test_cross_entropy_dice_needs_device_logits():
    from retinal_oct_image_segmentation_via_deep_learning_amd import OctError
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import cross_entropy_dice
    with pytest.raises(OctError, match="device tensor"):
        cross_entropy_dice(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
