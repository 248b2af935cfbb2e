"""CPU: what the four evaluators of evaluation.py share -- the image chunks under a workspace limit, the cached workspace, the
device rules of _Evaluator._bind, the summable state of _StateEvaluator before any update, and the model dispatch."""
import itertools

import numpy as np
import pytest
import torch

from retinal_oct_image_segmentation_via_deep_learning_amd import OctError
from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation as E

Z = torch.zeros(2, 4, 5, dtype=torch.int64)
# class, constructor arguments, a CPU update that passes every check but the device's, compute() on the zero state
EVALUATORS = {
    "SegEvaluator": (E.SegEvaluator, (3,), (Z, Z), lambda: E.metrics_from_state(np.zeros(E.state_size(3), np.int64), 3)),
    "BoundaryEvaluator": (E.BoundaryEvaluator, (3,), (Z, Z),
                          lambda: E.contour_metrics_from_records(np.zeros((0, 3, 2, 5), np.int64))),
    "ScoreEvaluator": (E.ScoreEvaluator, (2,), (torch.zeros(2, 2, 4, 5, dtype=torch.uint8), torch.zeros(2, 2, 4, 5)),
                       lambda: E.score_metrics_from_state(np.zeros(E.score_state_size(2), np.int64), 2, (0.5,), True)),
    "LesionEvaluator": (E.LesionEvaluator, (3,), (Z, Z),
                        lambda: E.lesion_metrics_from_state(np.zeros(E.lesion_state_size(3), np.int64), 3)),
}


def _holds_nothing(ev):
    return ev._chunks == [] if isinstance(ev, E.BoundaryEvaluator) else ev.state is None


def test_image_chunks_cover_the_batch_in_order_within_both_limits():
    grid = itertools.product((1, 2, 7, 33), (1, 1000), (1, 3, None), ((1, 1), (4, 5), (16384, 16384)))
    for images, one, factor, (h, w) in grid:
        limit = 10 ** 9 if factor is None else factor * one
        chunks = list(E._image_chunks(images, h, w, one, limit))
        assert [lo for lo, _ in chunks] == [sum(k for _, k in chunks[:i]) for i in range(len(chunks))]   # contiguous, in order
        assert sum(k for _, k in chunks) == images                                                       # [0, images) exactly
        for lo, k in chunks:
            assert 1 <= k <= limit // one and k * h * w < 2 ** 31, (images, one, limit, h, w, lo, k)
        # every chunk but the last is as large as a limit allows: one more image would break one of them
        sizes = [k for _, k in chunks]
        assert len(set(sizes[:-1])) <= 1 and sizes[-1] <= sizes[0]
        k = sizes[0]
        assert k == images or k + 1 > limit // one or (k + 1) * h * w >= 2 ** 31
        if (h, w) == (16384, 16384):
            assert k <= 7                                        # 8 * 2^28 pixels is 2^31
        if limit == one:
            assert sizes == [1] * images


def test_an_image_that_does_not_fit_the_workspace_raises_before_the_first_chunk():
    for one, limit in ((2, 1), (1000, 999), (10 ** 9 + 1, 10 ** 9)):
        with pytest.raises(RuntimeError, match=f"one 4 x 5 image needs a workspace of {one} bytes, max_workspace_bytes is {limit}"):
            E._image_chunks(3, 4, 5, one, limit)


def test_grown_keeps_a_buffer_that_is_large_enough():
    cpu = torch.device("cpu")
    buf = E._grown(None, 100, cpu)
    assert buf.dtype == torch.uint8 and buf.numel() == 100 and buf.device == cpu
    assert E._grown(buf, 100, cpu) is buf and E._grown(buf, 1, cpu) is buf
    more = E._grown(buf, 101, cpu)
    assert more is not buf and more.numel() == 101
    assert E._grown(buf, 100, torch.device("meta")) is not buf   # another device: a new buffer there
    assert E._grown(buf, 100, torch.device("meta")).device.type == "meta"


@pytest.mark.parametrize("name", EVALUATORS)
def test_before_any_update(name):
    cls, args, cpu_update, zero = EVALUATORS[name]
    with pytest.raises(OctError, match=f"{name} needs a GPU device: there is no CPU fallback on the product path"):
        cls(*args, device="cpu")
    ev = cls(*args)
    assert ev.device is None and cls(*args, device="cuda:1").device == torch.device("cuda", 1)
    assert ev.reset() is ev and _holds_nothing(ev)
    if isinstance(ev, E._StateEvaluator):                        # BoundaryEvaluator's records are not summable: no all_reduce
        assert ev.all_reduce() is ev and _holds_nothing(ev)
        assert ev._host_state().dtype == np.int64 and not ev._host_state().any() and _holds_nothing(ev)
    np.testing.assert_equal(ev.compute(), zero())
    with pytest.raises(OctError, match="no CPU fallback"):
        ev.update(*cpu_update)
    assert _holds_nothing(ev)


def test_the_class_tree():
    for cls in (E.SegEvaluator, E.ScoreEvaluator, E.LesionEvaluator):
        assert issubclass(cls, E._StateEvaluator) and "all_reduce" not in vars(cls) and "_state_on" not in vars(cls)
    assert issubclass(E._StateEvaluator, E._Evaluator) and issubclass(E.BoundaryEvaluator, E._Evaluator)
    assert not issubclass(E.BoundaryEvaluator, E._StateEvaluator) and not hasattr(E.BoundaryEvaluator, "all_reduce")


def test_bind_holds_the_three_device_rules():
    """torch.device values and a CPU tensor are enough: nothing here touches a GPU"""
    cuda0, cuda1 = torch.device("cuda", 0), torch.device("cuda", 1)
    held = torch.zeros(1, dtype=torch.int64)
    for ev in (E.SegEvaluator(3, device="cuda:1"), E.BoundaryEvaluator(3, device=cuda1)):
        with pytest.raises(OctError, match="no CPU fallback"):
            ev._bind(torch.device("cpu"), None, "state")
        with pytest.raises(RuntimeError, match="inputs are on cuda:0, the evaluator was made for cuda:1"):
            ev._bind(cuda0, None, "state")
        with pytest.raises(RuntimeError, match="inputs are on cuda:1, the evaluator's records on cpu"):
            ev._bind(cuda1, held, "records")
        ev._bind(cuda1, None, "state")
    E.LesionEvaluator(3, device="cuda")._bind(cuda0, None, "state")   # made for "a GPU", no index: any of them
    ev = E.SegEvaluator(3)
    ev.state = held
    with pytest.raises(RuntimeError, match="inputs are on cuda:0, the evaluator's state on cpu"):
        ev._state_on(cuda0)
    assert ev.state is held


def test_class_map_pair_and_element_codes():
    t = torch.zeros(2, 3, 4, 5, dtype=torch.int32)
    p = torch.zeros(2, 3, 4, 5, dtype=torch.bool)
    ct, cp, geometry = E._class_map_pair(t, p)
    assert geometry == (6, 4, 5) and ct.dtype == torch.int64 and cp.dtype == torch.uint8
    assert (E._elem(ct), E._elem(cp)) == (2, 0)
    assert E._class_map_pair(t[:0], p[:0])[2] == (0, 4, 5)
    with pytest.raises(RuntimeError, match="contour metrics take H, W <= 4, got 4 x 5"):
        E._class_map_pair(t, p, 4, "contour metrics")
    assert E._class_map_pair(t, p, 5, "contour metrics")[2] == (6, 4, 5)
    with pytest.raises(RuntimeError, match="H, W >= 1"):
        E._class_map_pair(t[..., :0], p[..., :0])


def test_model_kind():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    with pytest.raises(TypeError, match="update_model takes one of this package's networks, got Conv2d"):
        E._model_kind(torch.nn.Conv2d(1, 8, 1))
    assert E._model_kind(UNet(1, 8, init_features=4)) == (8, False)
    assert E._model_kind(M.MGUNet_2(1, 3, feature_scale=16)) == (3, True)


def test_int_and_state_checks():
    E._check_int("classes", 16, 1, 16)
    E._check_int("ignore_index", None, 0, 1, True)
    with pytest.raises(TypeError, match="classes must be an int, got NoneType None"):
        E._check_int("classes", None, 1, 16)
    with pytest.raises(TypeError, match="ignore_index must be an int or None, got bool True"):
        E._check_int("ignore_index", True, 0, 1, True)
    with pytest.raises(ValueError, match=r"classes must be in 1\.\.16 \(got 17\)"):
        E._check_int("classes", 17, 1, 16)
    s = E._int_state(np.arange(6, dtype=np.uint8).reshape(2, 3), 6, "x")
    assert s.dtype == np.int64 and s.shape == (6,)
    with pytest.raises(ValueError, match="state must hold 6 integers for 3 things, got float64 x 6"):
        E._int_state(np.zeros(6), 6, "3 things")
