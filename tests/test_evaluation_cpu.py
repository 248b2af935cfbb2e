"""CPU: the streaming evaluator's host side.  `metrics_from_state` against SURVEY App. B's known answers and against the
formulas of Metrics._formulas on independently counted sums; tests/eval_ref.py (the restatement the GPU tests compare with)
against a per-pixel loop; argument errors that need no device; the new export."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_ref as R
from retinal_oct_image_segmentation_via_deep_learning_amd import Metrics, OctError, _lib
from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation as E

YT = np.array([[1, 1, 0, 0], [1, 0, 0, 0]])
YP = np.array([[1, 0, 1, 0], [1, 0, 0, 1]])


def _loop_state(t, p, classes, ignore_index):
    """eval_ref.eval_state restated pixel by pixel"""
    h, w = t.shape[-2:]
    t, p = t.reshape(-1, h, w), p.reshape(-1, h, w)
    cc = classes * classes
    s = np.zeros(R.state_size(classes), dtype=np.int64)
    for b in range(t.shape[0]):
        for x in range(w):
            col = np.zeros(classes, dtype=np.int64)
            for y in range(h):
                tt, pp = int(t[b, y, x]), int(p[b, y, x])
                if ignore_index is not None and tt == ignore_index:
                    s[cc + classes + 1] += 1
                elif not (0 <= tt < classes and 0 <= pp < classes):
                    s[cc + classes + 2] += 1
                else:
                    s[tt * classes + pp] += 1
                    col[tt] += 1
                    col[pp] -= 1
            s[cc:cc + classes] += np.abs(col)
    s[cc + classes] = t.shape[0] * w
    s[cc + classes + 3] = 1
    return s


def test_survey_known_answers():
    m = E.metrics_from_state(R.eval_state(YT, YP, 2), 2)
    assert m["dice_coefficient"][1] == 0.5714285632653062
    assert m["iou_score"][1] == 0.39999999200000014
    assert m["specificity"][1] == 0.5999999880000002
    assert m["precision"][1] == 0.4999999875000003 and m["recall"][1] == 0.6666666444444452 and m["accuracy"][1] == 0.625
    assert m["thickness_error"][1] == 0.75
    np.testing.assert_array_equal(m["confusion"], [[3, 2], [1, 2]])
    np.testing.assert_array_equal(m["counts"][1], [2, 3, 4, 3, 2, 1])      # tp, t, p, tn, fp, fn
    assert (m["n"], m["ignored"], m["invalid"], m["columns"], m["updates"]) == (8, 0, 0, 4, 1)
    assert m["pixel_accuracy"] == 5 / 8
    assert m["thickness_error"][1] == R.thickness_difference(YT == 1, YP == 1)


@pytest.mark.parametrize("classes,ignore", [(1, None), (3, None), (5, 255), (16, -100)])
def test_restatement_matches_a_per_pixel_loop(classes, ignore):
    rng = np.random.default_rng(classes)
    t = rng.integers(0, classes, size=(2, 3, 6, 9))
    p = rng.integers(0, classes, size=t.shape)
    t[rng.random(t.shape) < 0.1] = classes + 2          # out of range on the target side
    p[rng.random(t.shape) < 0.1] = -1                   # and on the prediction side
    if ignore is not None:
        t[rng.random(t.shape) < 0.2] = ignore
    got = R.eval_state(t, p, classes, ignore)
    np.testing.assert_array_equal(got, _loop_state(t, p, classes, ignore))
    assert got[:classes * classes].sum() + got[-3] + got[-2] == t.size


def test_formulas_are_the_package_formulas_on_reference_counts():
    rng = np.random.default_rng(7)
    t, p = R.layered_maps(rng, (3, 40, 50), 6)
    s = R.eval_state(t, p, 6)
    m = E.metrics_from_state(s, 6)
    counts = R.one_vs_rest_counts(s[:36].reshape(6, 6))
    np.testing.assert_array_equal(m["counts"], counts)
    for c in range(6):
        assert counts[c, 1] == (t == c).sum() and counts[c, 2] == (p == c).sum() and counts[c, 0] == ((t == c) & (p == c)).sum()
        ref = Metrics._formulas(*(int(v) for v in counts[c]), int(t.size))
        for k, v in ref.items():
            assert m[k][c] == v, (k, c)
        assert m["thickness_error"][c] == s[36 + c] / (3 * 50)


def test_absent_classes_are_left_out_of_the_means():
    t = np.array([[0, 0, 2, 2], [0, 2, 2, 2]])
    p = np.array([[0, 2, 2, 2], [0, 2, 2, 0]])
    m = E.metrics_from_state(R.eval_state(t, p, 4), 4)
    np.testing.assert_array_equal(m["present"], [True, False, True, False])
    assert m["dice_coefficient"][1] == 0.0 and m["dice_coefficient"][3] == 0.0
    assert m["mean_dice"] == (m["dice_coefficient"][0] + m["dice_coefficient"][2]) / 2
    assert m["mean_iou"] == (m["iou_score"][0] + m["iou_score"][2]) / 2
    assert m["mean_dice"] > m["dice_coefficient"].mean()


def test_empty_state_gives_nan_not_an_error():
    m = E.metrics_from_state(np.zeros(R.state_size(3), dtype=np.int64), 3)
    assert m["columns"] == 0 and np.isnan(m["thickness_error"]).all() and m["thickness_error"].shape == (3,)
    assert np.isnan(m["pixel_accuracy"]) and np.isnan(m["mean_dice"]) and np.isnan(m["accuracy"]).all()
    assert not m["present"].any() and m["n"] == 0
    fresh = E.SegEvaluator(3).compute()                  # nothing updated: no state, no device needed
    assert fresh["updates"] == 0 and np.isnan(fresh["thickness_error"]).all()


def test_everything_ignored_counts_nowhere_else():
    t = np.full((2, 4, 5), 255)
    s = R.eval_state(t, np.zeros_like(t), 3, 255)
    m = E.metrics_from_state(s, 3)
    assert m["ignored"] == 40 and m["n"] == 0 and m["invalid"] == 0 and not m["confusion"].any()
    assert (m["thickness_error"] == 0).all() and m["columns"] == 10


def test_state_size_and_layout_agree_with_the_header():
    assert E.state_size(8) == R.state_size(8) == 8 * 8 + 8 + 4 and _lib.EVAL_STATE_EXTRA == 4
    assert C.sizeof(_lib.SegEvalDesc) == 40 and _lib.SegEvalDesc.ignore_index.offset == 32


def test_argument_errors_need_no_gpu():
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="classes must be in 1..16"):
            E.SegEvaluator(bad)
    for bad in ("3", 3.0, True, None):
        with pytest.raises(TypeError, match="classes must be an int"):
            E.SegEvaluator(bad)
    for bad in (1.5, "255", True):
        with pytest.raises(TypeError, match="ignore_index must be an int or None"):
            E.SegEvaluator(3, ignore_index=bad)
    with pytest.raises(ValueError, match="not an int64"):
        E.SegEvaluator(3, ignore_index=2 ** 63)
    with pytest.raises(OctError, match="no CPU fallback"):
        E.SegEvaluator(3, device="cpu")
    ev = E.SegEvaluator(3, ignore_index=255)
    t = torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="same shape"):
        ev.update(t, torch.zeros(2, 5, 4, dtype=torch.int64))
    with pytest.raises(TypeError, match="integer class map"):
        ev.update(t, torch.zeros(2, 4, 5))
    with pytest.raises(TypeError, match="torch tensor"):
        ev.update(t, np.zeros((2, 4, 5), dtype=np.int64))
    with pytest.raises(RuntimeError, match=r"\(\.\.\., H, W\)"):
        ev.update(torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64))
    with pytest.raises(OctError, match="no CPU fallback"):
        ev.update(t, t)
    with pytest.raises(ValueError, match="layout"):
        ev.update_logits(t, torch.zeros(2, 4, 5, 3), "hwc")
    with pytest.raises(RuntimeError, match="4 channels, the evaluator 3"):
        ev.update_logits(t, torch.zeros(2, 4, 5, 4), "nhwc")
    with pytest.raises(OctError, match="NCHW logits must be fp32"):
        ev.update_logits(t, torch.zeros(2, 3, 4, 5, dtype=torch.bfloat16), "nchw")
    with pytest.raises(OctError, match="NHWC logits must be bf16 or fp32"):
        ev.update_logits(t, torch.zeros(2, 4, 5, 3, dtype=torch.float16), "nhwc")
    with pytest.raises(RuntimeError, match="target must have shape"):
        ev.update_logits(torch.zeros(2, 5, 4, dtype=torch.int64), torch.zeros(2, 4, 5, 3), "nhwc")
    with pytest.raises(RuntimeError, match="expected 4-D logits"):
        ev.update_logits(t, torch.zeros(4, 5, 3), "nhwc")
    with pytest.raises(OctError, match="no CPU fallback"):
        ev.update_logits(t, torch.zeros(2, 4, 5, 3), "nhwc")
    assert ev.state is None                              # nothing was allocated or launched
    with pytest.raises(ValueError, match="state must hold 16 integers"):
        E.metrics_from_state(np.zeros(15, dtype=np.int64), 3)
    with pytest.raises(ValueError, match="state must hold"):
        E.metrics_from_state(np.zeros(16), 3)
    with pytest.raises(TypeError, match="integer arrays"):
        Metrics.confusion_matrix(np.zeros((2, 2)), np.zeros((2, 2)), 2)
    with pytest.raises(ValueError, match="classes must be in"):
        Metrics.confusion_matrix(YT, YP, 17)


def test_update_model_checks_before_the_forward():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    net, lg = UNet(1, 8, init_features=4).eval(), M.MGUNet_2(1, 3, feature_scale=16).eval()
    x = torch.zeros(2, 1, 32, 32)
    with pytest.raises(TypeError, match="one of this package's networks"):
        E.SegEvaluator(8).update_model(torch.nn.Conv2d(1, 8, 1), x, torch.zeros(2, 32, 32, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="UNet has 8 classes, the evaluator 3"):
        E.SegEvaluator(3).update_model(net, x, torch.zeros(2, 32, 32, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="MGUNet_2 has 3 classes, the evaluator 8"):
        E.SegEvaluator(8).update_model(lg, x, torch.zeros(2, 32, 32, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"target must have shape \(2, 32, 32\)"):
        E.SegEvaluator(8).update_model(net, x, torch.zeros(2, 1, 32, 32, dtype=torch.int64))
    with pytest.raises(TypeError, match="integer class map"):
        E.SegEvaluator(3).update_model(lg, x, torch.zeros(2, 32, 32))


def test_all_reduce_is_a_no_op_in_one_process():
    ev = E.SegEvaluator(2)
    assert ev.all_reduce() is ev and ev.state is None


def test_the_library_exports_the_entry_point_and_validates_on_the_host():
    lib = _lib.lib()
    assert "oct_seg_eval_update" in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), "oct_seg_eval_update")
    assert lib.oct_version() == 220
    assert lib.oct_seg_eval_update(None, None, None, None, None) == -22 and "null descriptor" in _lib.last_error()
    buf = (C.c_int64 * 1024)()
    one = C.addressof(buf)

    def call(**kw):
        f = dict(images=1, h=2, w=2, classes=3, target_elem=2, pred_kind=1, has_ignore=0, ignore_index=0)
        f.update(kw)
        d = _lib.SegEvalDesc(*(f[k] for k, _ in _lib.SegEvalDesc._fields_))
        return lib.oct_seg_eval_update(C.byref(d), one, one, one, None)

    for kw, msg in (({"classes": 0}, "classes must be 1..16"), ({"classes": 17}, "classes must be 1..16"),
                    ({"h": 0}, "bad geometry"), ({"w": -3}, "bad geometry"), ({"images": 1 << 20, "h": 1 << 10, "w": 2}, "below 2\\^31"),
                    ({"target_elem": 1}, "uint8 \\(0\\) or int64 \\(2\\)"), ({"pred_kind": 5}, "bad pred_kind"),
                    ({"pred_kind": -1}, "bad pred_kind")):
        assert call(**kw) == -22, kw
        import re
        assert re.search(msg, _lib.last_error()), (kw, _lib.last_error())
    d = _lib.SegEvalDesc(1, 2, 2, 3, 2, 1, 0, 0)
    assert lib.oct_seg_eval_update(C.byref(d), one, one, None, None) == -22 and "null state" in _lib.last_error()
    assert lib.oct_seg_eval_update(C.byref(d), one + 4, one, one, None) == -22 and "8-byte aligned" in _lib.last_error()
