"""CPU: the connected-component restatement (tests/cc_ref.py) against scipy.ndimage.label and on known answers, the host formulas
evaluation.lesion_metrics_from_state, the argument errors of postprocess / LesionEvaluator, and the C-ABI symbols without a GPU
(workspace formula, rejected descriptors).  Everything is integers: every comparison is ==."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cc_ref as R

B = 1 << R.BORDER_BIT


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


def _P():
    from retinal_oct_image_segmentation_via_deep_learning_amd import postprocess
    return postprocess


# ---- the restatement against scipy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_scipy_label(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else None
    rng = np.random.default_rng(11)
    maps = [rng.integers(0, 3, size=s) for s in ((1, 1), (1, 9), (7, 1), (5, 6), (33, 40), (67, 130))]
    maps += [(rng.random((67, 130)) < 0.59).astype(np.int64), R.serpentine(65, 130), R.spiral(40, 67)]
    for m in maps:
        roots, info = R.label(m, 3, connectivity)
        assert (roots >= 0).all()
        for c in range(3):
            lab, n = ndi.label(m == c, structure=structure)
            mine = roots[m == c]
            order = np.unique(mine)                      # ascending roots of the class
            assert len(order) == n
            # equal partitions, and ascending root = scipy's numbering 1..n
            np.testing.assert_array_equal(np.searchsorted(order, mine) + 1, lab[m == c])
            ry, rx = np.divmod(order, m.shape[1])
            np.testing.assert_array_equal(info[ry, rx] & (B - 1), np.bincount(lab[m == c], minlength=n + 1)[1:])
        assert (info != 0).sum() == len(np.unique(roots))


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_checkerboard_singletons_at_4_two_components_at_8():
    m = np.indices((6, 7)).sum(axis=0) % 2
    roots, info = R.label(m, 2, 4)
    np.testing.assert_array_equal(roots, np.arange(42).reshape(6, 7))
    assert ((info & (B - 1)) == 1).all()
    roots, info = R.label(m, 2, 8)
    np.testing.assert_array_equal(roots, m)              # class 0 hangs on pixel 0, class 1 on pixel 1
    assert info[0, 0] == (21 | B) and info[0, 1] == (21 | B) and (info != 0).sum() == 2
    t = R.table(m, 2, 8)
    np.testing.assert_array_equal(t, [[0, 0, 0, 0, 21, 1], [0, 1, 0, 1, 21, 1]])


def _rings():
    m = np.zeros((9, 9), dtype=np.int64)
    m[1:8, 1:8] = 1
    m[2:7, 2:7] = 0
    m[3:6, 3:6] = 1
    m[4, 4] = 0
    return m


def test_concentric_rings_enclosed_flags_and_hole_filling():
    m = _rings()
    t = R.table(m, 2, 4)
    # class 0: the frame (touches), the gap between the rings (enclosed), the centre pixel (enclosed); class 1: two rings
    np.testing.assert_array_equal(t, [[0, 0, 0, 0, 32, 1], [0, 0, 2, 2, 16, 0], [0, 0, 4, 4, 1, 0],
                                      [0, 1, 1, 1, 24, 0], [0, 1, 3, 3, 8, 0]])
    filled = R.filter_map(m, 2, fill_enclosed=[1, 0], replace=[1, 0])
    want = np.zeros((9, 9), dtype=np.int64)
    want[1:8, 1:8] = 1
    np.testing.assert_array_equal(filled, want)
    # one pass: dropping the enclosed class-1 rings does not look at what that uncovers
    np.testing.assert_array_equal(R.filter_map(m, 2, fill_enclosed=[0, 1], replace=0), np.zeros((9, 9), dtype=np.int64))


def test_equal_area_tie_keeps_the_smaller_root_and_min_area_is_inclusive():
    m = np.zeros((5, 9), dtype=np.int64)
    m[1, 1:4] = 1          # root 10, area 3
    m[3, 5:8] = 1          # root 32, area 3
    m[3, 1] = 1            # root 28, area 1
    out = R.filter_map(m, 2, keep_largest=[0, 1])
    want = np.zeros_like(m)
    want[1, 1:4] = 1
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(R.filter_map(m, 2, min_area=[0, 3]), np.where(np.arange(45).reshape(5, 9) == 28, 0, m))
    np.testing.assert_array_equal(R.filter_map(m, 2, min_area=[0, 4]), np.zeros_like(m))
    np.testing.assert_array_equal(R.filter_map(m, 2, min_area=1), m)
    # an outside pixel is copied and splits a component
    m2 = m.copy()
    m2[1, 2] = 7
    out = R.filter_map(m2, 2, min_area=[0, 2], ignore_index=None)
    want = np.zeros_like(m)
    want[1, 2] = 7
    want[3, 5:8] = 1
    np.testing.assert_array_equal(out, want)


def test_overlap_rule_counts_equality_as_detected():
    t = np.zeros((1, 4, 8), dtype=np.int64)
    p = np.zeros((1, 4, 8), dtype=np.int64)
    t[0, 1, 1:5] = 1                                    # area 4
    p[0, 1, 4:6] = 1                                    # inter 1; the predicted component has area 2
    s = R.lesion_state(t, p, 2, min_overlap=(1, 4))     # 1 * 4 >= 1 * 4: detected; 1 * 4 >= 1 * 2: confirmed
    np.testing.assert_array_equal(s[4:8], [1, 1, 1, 1])
    s = R.lesion_state(t, p, 2, min_overlap=(1, 2))     # 1 * 2 < 1 * 4: missed; 1 * 2 >= 1 * 2: confirmed
    np.testing.assert_array_equal(s[4:8], [1, 1, 0, 1])
    s = R.lesion_state(t, p, 2, min_overlap=(3, 4))
    np.testing.assert_array_equal(s[4:8], [1, 1, 0, 0])
    s = R.lesion_state(t, np.zeros_like(p), 2)          # no overlap at all: inter >= 1 fails even with 0 / 1
    np.testing.assert_array_equal(s[4:8], [1, 0, 0, 0])
    np.testing.assert_array_equal(s[8:], [1, 0, 0, 1])


def test_ignored_target_pixel_splits_a_predicted_component():
    t = np.zeros((3, 7), dtype=np.int64)
    p = np.zeros((3, 7), dtype=np.int64)
    p[1, 1:6] = 1
    t[1, 3] = 255
    t[1, 5] = 1
    p[0, 0] = 9                                         # invalid: outside [0, 2), not ignored
    s = R.lesion_state(t, p, 2, ignore_index=255)
    # class 1: one target component (detected), two predicted pieces, the right one confirmed
    np.testing.assert_array_equal(s[4:8], [1, 2, 1, 1])
    np.testing.assert_array_equal(s[8:], [1, 1, 1, 1])


# ---- host formulas ----------------------------------------------------------------------------------------------------------
def test_lesion_metrics_formulas_and_nan_cases():
    E = _E()
    state = np.array([4, 5, 3, 2,   0, 0, 0, 0,   2, 0, 0, 0,   3, 2, 0, 0,   7, 11, 13, 3], dtype=np.int64)
    m = E.lesion_metrics_from_state(state, 4)
    np.testing.assert_array_equal(m["target_components"], [4, 0, 2, 3])
    np.testing.assert_array_equal(m["confirmed"], [2, 0, 0, 0])
    assert m["sensitivity"][0] == 3 / 4 and m["precision"][0] == 2 / 5
    assert m["f1"][0] == 2 * (3 / 4) * (2 / 5) / (3 / 4 + 2 / 5)
    assert np.isnan(m["sensitivity"][1]) and np.isnan(m["precision"][1]) and np.isnan(m["f1"][1])
    assert m["sensitivity"][2] == 0.0 and np.isnan(m["precision"][2]) and np.isnan(m["f1"][2])
    assert m["sensitivity"][3] == 0.0 and m["precision"][3] == 0.0 and m["f1"][3] == 0.0
    assert (m["images"], m["ignored"], m["invalid"], m["updates"]) == (7, 11, 13, 3)
    assert m["f1"].dtype == np.float64
    with pytest.raises(ValueError, match="state"):
        E.lesion_metrics_from_state(state[:-1], 4)
    with pytest.raises(ValueError, match="state"):
        E.lesion_metrics_from_state(state.astype(np.float64), 4)
    z = E.LesionEvaluator(3).compute()
    assert z["updates"] == 0 and np.isnan(z["f1"]).all()


# ---- argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors(L):
    E, P = _E(), _P()
    for bad in (0, 17):
        with pytest.raises(ValueError, match="classes"):
            E.LesionEvaluator(bad)
        with pytest.raises(ValueError, match="classes"):
            P.ComponentFilter(bad)
    with pytest.raises(TypeError, match="classes"):
        P.ComponentFilter(2.0)
    with pytest.raises(TypeError, match="ignore_index"):
        E.LesionEvaluator(2, ignore_index=1.5)
    for bad in (6, True, "8"):
        with pytest.raises(ValueError, match="connectivity"):
            E.LesionEvaluator(2, connectivity=bad)
        with pytest.raises(ValueError, match="connectivity"):
            P.ComponentFilter(2, connectivity=bad)
    for bad in ((1, 0), (2, 1), (-1, 2)):
        with pytest.raises(ValueError, match="min_overlap"):
            E.LesionEvaluator(2, min_overlap=bad)
    for bad in (0.5, (1.0, 2), (1, 2, 3)):
        with pytest.raises(TypeError, match="min_overlap"):
            E.LesionEvaluator(2, min_overlap=bad)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        E.LesionEvaluator(2, max_workspace_bytes=0)
    with pytest.raises(L.OctError, match="GPU"):
        E.LesionEvaluator(2, device="cpu")
    with pytest.raises(ValueError, match="min_area"):
        P.ComponentFilter(3, min_area=[1, 2])
    with pytest.raises(ValueError, match="min_area"):
        P.ComponentFilter(3, min_area=-1)
    with pytest.raises(TypeError, match="min_area"):
        P.ComponentFilter(3, min_area=1.5)
    with pytest.raises(ValueError, match="keep_largest"):
        P.ComponentFilter(3, keep_largest=2)
    with pytest.raises(ValueError, match="fill_enclosed"):
        P.ComponentFilter(3, fill_enclosed=[0, 1, 2])
    flt = P.ComponentFilter(3, min_area=4, keep_largest=[0, 1, True], replace=[0, 0, 300])
    assert flt.min_area == [4, 4, 4] and flt.keep_largest == [0, 1, 1] and flt.fill_enclosed == [0, 0, 0]
    z = torch.zeros(2, 4, 5, dtype=torch.int64)
    ev = E.LesionEvaluator(3)
    with pytest.raises(TypeError, match="integer class map"):
        ev.update(z.float(), z)
    with pytest.raises(TypeError, match="torch tensor"):
        ev.update(z.numpy(), z)
    with pytest.raises(RuntimeError, match="same shape"):
        ev.update(z, z[:, :, :4])
    with pytest.raises(L.OctError, match="no CPU fallback"):
        ev.update(z, z)
    with pytest.raises(TypeError, match="networks"):
        ev.update_model(torch.nn.Conv2d(1, 3, 1), z, z)
    tall = torch.zeros(1, 16385, 1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="16384"):
        ev.update(tall, tall)
    with pytest.raises(RuntimeError, match="16384"):
        P.connected_components(tall, 2)
    with pytest.raises(TypeError, match="integer class map"):
        P.connected_components(z.float(), 2)
    with pytest.raises(RuntimeError, match=r"\(\.\.\., H, W\)"):
        flt(z[0, 0])
    with pytest.raises(L.OctError, match="no CPU fallback"):
        P.connected_components(z, 3)
    with pytest.raises(L.OctError, match="no CPU fallback"):
        flt(z)
    with pytest.raises(ValueError, match="uint8"):
        flt(z.to(torch.uint8))                           # replace 300 does not fit
    with pytest.raises(RuntimeError, match="two-class"):
        flt.filter_masks(torch.zeros(1, 2, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"\(B, C, H, W\)"):
        P.ComponentFilter(2).filter_masks(torch.zeros(2, 4, 4, dtype=torch.uint8))


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------
def _desc(L, images=3, h=33, w=130, classes=9, map_elem=0, pred_elem=2, conn=4, op=0, has_ignore=1, num=0, den=1, ignore=255):
    return L.CcDesc(images, h, w, classes, map_elem, pred_elem, conn, op, has_ignore, num, den, 0, ignore)


def test_abi_workspace_formula_and_rejected_descriptors(L):
    lib = L.lib()

    def up(v):
        return (v + 255) // 256 * 256

    n = 3 * 33 * 130
    assert lib.oct_cc_workspace_bytes(C.byref(_desc(L, op=L.CC_OP_LABEL))) == up(n)
    assert lib.oct_cc_workspace_bytes(C.byref(_desc(L, op=L.CC_OP_FILTER))) == up(n) + up(8 * 3 * 9)
    want = 2 * up(n) + 6 * up(4 * n)
    assert lib.oct_cc_workspace_bytes(C.byref(_desc(L, op=L.CC_OP_LESION))) == want
    one = lib.oct_cc_workspace_bytes(C.byref(_desc(L, images=1, op=L.CC_OP_LESION)))
    assert 0 < one and 3 * one >= want                   # the chunking rule: bytes(k) <= k * bytes(1)
    th, tw = C.c_int(0), C.c_int(0)
    assert lib.oct_cc_tile(C.byref(th), C.byref(tw)) == 0 and th.value >= 1 and tw.value >= 1
    assert lib.oct_cc_tile(None, None) == -22
    rules = L.CcRules()
    bad = ((_desc(L, h=16385), "16384"), (_desc(L, w=16385), "16384"), (_desc(L, classes=17), "classes"),
           (_desc(L, classes=0), "classes"), (_desc(L, map_elem=1), "uint8"), (_desc(L, pred_elem=3), "uint8"),
           (_desc(L, h=0), "geometry"), (_desc(L, images=-1), "geometry"), (_desc(L, conn=6), "connectivity"),
           (_desc(L, op=3), "op"), (_desc(L, den=0), "overlap"), (_desc(L, num=2, den=1), "overlap"),
           (_desc(L, num=-1), "overlap"), (_desc(L, images=40000, h=16384, w=16384), "2^31"))
    for d, msg in bad:
        assert lib.oct_cc_workspace_bytes(C.byref(d)) == 0 and msg in L.last_error(), msg
        assert lib.oct_cc_label(C.byref(d), None, None, None, None, None) == -22 and msg in L.last_error()
        assert lib.oct_cc_filter(C.byref(d), C.byref(rules), None, None, None, None, None, None) == -22 and msg in L.last_error()
        assert lib.oct_lesion_eval_update(C.byref(d), None, None, None, None, None) == -22 and msg in L.last_error()
    assert lib.oct_cc_workspace_bytes(None) == 0 and "null descriptor" in L.last_error()
    d = _desc(L)
    assert lib.oct_cc_label(C.byref(d), None, None, None, None, None) == -22 and "null map" in L.last_error()
    assert lib.oct_lesion_eval_update(C.byref(d), None, None, None, None, None) == -22 and "null target" in L.last_error()
    assert lib.oct_cc_filter(C.byref(d), None, None, None, None, None, None, None) == -22 and "null rules" in L.last_error()
    rules.min_area[2] = -1
    assert lib.oct_cc_filter(C.byref(d), C.byref(rules), None, None, None, None, None, None) == -22 and "min_area" in L.last_error()
    rules.min_area[2] = 0
    rules.keep_largest[1] = 2
    assert lib.oct_cc_filter(C.byref(d), C.byref(rules), None, None, None, None, None, None) == -22 and "keep_largest" in L.last_error()
    rules.keep_largest[1] = 1
    rules.replace[0] = 256
    assert lib.oct_cc_filter(C.byref(d), C.byref(rules), None, None, None, None, None, None) == -22 and "uint8" in L.last_error()
