"""CPU: the distance-map restatement (tests/dt_ref.py) against scipy.ndimage.distance_transform_edt, against an all-pairs
minimum and on known answers; the tables of DistanceWeightMap against their formulas; the argument errors of the distance module
and the C-ABI symbols without a GPU (workspace formula, rejected descriptors).  Squared distances are integers: every comparison
of them is ==."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import dt_ref as R

PLANES = ["boundary", ("class", 0), ("class", 2), ("other", 1), ("other", 2)]


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


def _D():
    from retinal_oct_image_segmentation_via_deep_learning_amd import distance
    return distance


def _maps():
    """(map, classes, ignore_index): bands, noise of several densities, invalid and ignored pixels, degenerate shapes"""
    rng = np.random.default_rng(5)
    out = [(R.wavy_bands(rng, (70, 300), 6), 6, None), (rng.integers(0, 3, size=(40, 67)), 3, None),
           ((rng.random((70, 300)) < 0.01).astype(np.int64) * 2, 3, None), (rng.integers(0, 3, size=(1, 50)), 3, None),
           (rng.integers(0, 3, size=(50, 1)), 3, None), (np.full((9, 11), 2), 3, None)]
    m = rng.integers(0, 4, size=(33, 80))
    m[rng.random(m.shape) < 0.1] = 9                       # out of range
    m[5:20, 10:40] = 3                                     # an ignored rectangle
    out.append((m, 4, 3))
    return out


# ---- the restatement against scipy and against all pairs --------------------------------------------------------------------
def test_restatement_equals_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    checked = 0
    for m, classes, ignore in _maps():
        planes = ["boundary"] + [(k, c) for k in ("class", "other") for c in range(classes)]
        got = R.squared_distance(m, classes, planes, ignore)
        for p, plane in enumerate(planes):
            s = R.sites(m, classes, plane, ignore)
            if not s.any():
                assert (got[p] == R.FAR).all()
                continue
            _, idx = ndi.distance_transform_edt(~s, return_indices=True)
            yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
            want = (yy - idx[0]).astype(np.int64) ** 2 + (xx - idx[1]).astype(np.int64) ** 2   # integers from the indices
            np.testing.assert_array_equal(got[p], want, err_msg=f"{plane} {m.shape}")
            checked += 1
    assert checked >= 30


def test_restatement_equals_all_pairs_on_small_maps():
    rng = np.random.default_rng(6)
    for h, w in ((1, 1), (1, 12), (12, 1), (5, 7), (12, 12), (9, 12)):
        for density in (0.02, 0.3, 0.9):
            s = rng.random((h, w)) < density
            np.testing.assert_array_equal(R.squared_image(s), R.brute_force(s))
        m = rng.integers(0, 3, size=(h, w))
        m[rng.random((h, w)) < 0.15] = 7
        for plane in PLANES:
            np.testing.assert_array_equal(R.squared_distance(m, 3, [plane], 1)[0], R.brute_force(R.sites(m, 3, plane, 1)))
    wide = np.zeros((3, 200), dtype=bool)                  # more site columns than the column-by-column path takes
    wide[1, ::2] = True
    np.testing.assert_array_equal(R.squared_image(wide), R.brute_force(wide))


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_single_site_at_a_corner_no_site_and_a_vertical_split():
    h, w = 23, 41
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=np.int64)
    m[0, 0] = 1
    np.testing.assert_array_equal(R.squared_distance(m, 2, [("class", 1)])[0], yy ** 2 + xx ** 2)
    m = np.zeros((h, w), dtype=np.int64)
    m[h - 1, w - 1] = 1
    np.testing.assert_array_equal(R.squared_distance(m, 2, [("class", 1)])[0], (h - 1 - yy) ** 2 + (w - 1 - xx) ** 2)
    none = R.squared_distance(np.zeros((h, w), dtype=np.int64), 2, ["boundary", ("class", 1), ("other", 0)])
    assert none.dtype == np.int32 and (none == R.FAR).all() and R.FAR == 1 << 30
    x0 = 17                                                # columns 0..x0 are class 0, the rest class 1
    split = (xx > x0).astype(np.int64)
    want = np.minimum(np.abs(xx - x0), np.abs(xx - x0 - 1)) ** 2
    np.testing.assert_array_equal(R.squared_distance(split, 2, ["boundary"])[0], want)


def test_site_sets_edges_ignored_neighbours_and_invalid_pixels():
    m = np.array([[0, 0, 1, 1],
                  [0, 5, 1, 9],
                  [0, 0, 0, 1]])
    b = R.sites(m, 3, "boundary", ignore_index=None)       # 5 and 9 are out of range: no sites, and they make none
    np.testing.assert_array_equal(b, [[0, 1, 1, 0], [0, 0, 1, 0], [0, 0, 1, 1]])
    m2 = np.array([[0, 2, 1]])                             # the ignored pixel separates 0 from 1: no boundary at all
    assert not R.sites(m2, 3, "boundary", ignore_index=2).any()
    assert R.sites(m2, 3, "boundary").all()
    assert not R.sites(np.zeros((4, 4), dtype=np.int64), 2, "boundary").any()   # the image edge is no boundary
    np.testing.assert_array_equal(R.sites(m, 3, ("class", 1)), m == 1)
    np.testing.assert_array_equal(R.sites(m, 3, ("other", 1)), m == 0)          # 5 and 9 are not "other": invalid
    np.testing.assert_array_equal(R.sites(m, 3, ("other", 1), ignore_index=0), np.zeros_like(m, dtype=bool))
    d2 = R.squared_distance(m, 3, [("class", 1)])[0]
    assert d2[1, 1] == 1 and d2[1, 3] == 1                 # invalid pixels still receive a distance


def test_signed_map_and_table_lookup():
    m = np.zeros((5, 9), dtype=np.int64)
    m[:, 4:] = 1
    s = R.signed_distance(m, 3)                            # class 2 is absent; classes 0 and 1 split the image
    assert s.shape == (3, 5, 9) and s.dtype == np.float64 and not s[2].any()
    np.testing.assert_array_equal(s[0][0], [-4, -3, -2, -1, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(s[1], -s[0])
    assert not R.signed_distance(np.zeros((4, 4), dtype=np.int64), 2).any()      # nothing valid outside class 0
    m[0, 0] = 7                                            # an invalid pixel is outside every class and positive everywhere
    s = R.signed_distance(m, 3, [0, 1])
    assert s[0][0, 0] == 1.0 and s[1][0, 0] == 4.0 and s[0][0, 1] == -3.0        # ... and no site of "other"
    table = np.array([3.0, 2.0, 1.5, 1.0], dtype=np.float32)
    d2 = np.array([[0, 1, 2, 3, 4, 1 << 30]])
    np.testing.assert_array_equal(R.table_lookup(d2, table), np.array([[3.0, 2.0, 1.5, 1.0, 1.0, 1.0]], dtype=np.float32))
    assert R.table_lookup(d2, table).dtype == np.float32


# ---- the tables ------------------------------------------------------------------------------------------------------------
def test_gaussian_and_boundary_bonus_tables_equal_their_formulas():
    D = _D()
    for w0, sigma, base, cut in ((10.0, 5.0, 1.0, 4.0), (2.5, 1.3, 0.5, 3.0), (1.0, 0.25, 0.0, 1.0)):
        wm = D.DistanceWeightMap.gaussian(9, w0, sigma, base=base, cutoff_sigmas=cut, ignore_index=255)
        kmax = math.ceil(cut * sigma) ** 2
        want = [base + w0 * math.exp(-k / (2.0 * sigma * sigma)) for k in range(kmax + 1)] + [base]
        assert wm.table.dtype == torch.float32 and wm.table.shape == (kmax + 2,)
        np.testing.assert_array_equal(wm.table.numpy(), np.array(want, dtype=np.float64).astype(np.float32))
        assert wm.classes == 9 and wm.ignore_index == 255
    wm = D.DistanceWeightMap.gaussian(9, 10.0, 5.0)
    assert wm.table.shape == (402,) and wm.table[0] == 11.0 and wm.table[-1] == 1.0
    bb = D.DistanceWeightMap.boundary_bonus(4, 2.0, base=0.5)
    np.testing.assert_array_equal(bb.table.numpy(), np.array([2.5, 0.5], dtype=np.float32))
    t = D.DistanceWeightMap(3, torch.tensor([1.0, 0.1], dtype=torch.float64)).table
    np.testing.assert_array_equal(t.numpy(), np.array([1.0, 0.1], dtype=np.float32))   # rounded once, from float64


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_argument_errors(L):
    D = _D()
    m = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="classes"):
            D.squared_distance(m, bad, ["boundary"])
        with pytest.raises(ValueError, match="classes"):
            D.signed_distance(m, bad)
        with pytest.raises(ValueError, match="classes"):
            D.DistanceWeightMap(bad, [1.0])
    with pytest.raises(TypeError, match="classes"):
        D.squared_distance(m, 2.0, ["boundary"])
    with pytest.raises(TypeError, match="ignore_index"):
        D.squared_distance(m, 3, ["boundary"], ignore_index=1.5)
    with pytest.raises(ValueError, match="empty"):
        D.squared_distance(m, 3, [])
    with pytest.raises(TypeError, match="planes"):
        D.squared_distance(m, 3, "boundary")
    for bad in ("edge", ("class",), ("klass", 1), ("class", 1, 2), 3):
        with pytest.raises(ValueError, match="a plane is"):
            D.squared_distance(m, 3, [bad])
    for bad in (3, -1):
        with pytest.raises(ValueError, match="class of plane"):
            D.squared_distance(m, 3, [("class", bad)])
        with pytest.raises(ValueError, match="class of plane"):
            D.squared_distance(m, 3, ["boundary", ("other", bad)])
        with pytest.raises(ValueError, match="class_ids"):
            D.signed_distance(m, 3, [0, bad])
    with pytest.raises(TypeError, match="class of plane"):
        D.squared_distance(m, 3, [("class", True)])
    with pytest.raises(ValueError, match="at most 64"):
        D.squared_distance(m, 3, ["boundary"] * 65)
    with pytest.raises(ValueError, match="class_ids is empty"):
        D.signed_distance(m, 3, [])
    with pytest.raises(ValueError, match="at most 32"):
        D.signed_distance(m, 3, [0] * 33)
    with pytest.raises(ValueError, match="table is empty"):
        D.DistanceWeightMap(3, [])
    with pytest.raises(ValueError, match="table is empty"):
        D.DistanceWeightMap(3, torch.zeros(0))
    with pytest.raises(ValueError, match="finite"):
        D.DistanceWeightMap(3, [1.0, float("nan")])
    with pytest.raises(TypeError, match="table"):
        D.DistanceWeightMap(3, 1.0)
    with pytest.raises(ValueError, match="sigma"):
        D.DistanceWeightMap.gaussian(3, 1.0, 0.0)
    with pytest.raises(TypeError, match="w0"):
        D.DistanceWeightMap.gaussian(3, "1", 1.0)
    with pytest.raises(TypeError, match="w1"):
        D.DistanceWeightMap.boundary_bonus(3, None)
    wm = D.DistanceWeightMap.boundary_bonus(3, 1.0)
    calls = (lambda t: D.squared_distance(t, 3, ["boundary"]), lambda t: D.signed_distance(t, 3), wm)
    for call in calls:
        with pytest.raises(TypeError, match="integer class map"):
            call(torch.zeros(2, 8, 8))
        with pytest.raises(TypeError, match="torch tensor"):
            call(np.zeros((8, 8), dtype=np.int64))
        with pytest.raises(RuntimeError, match=r"\(\.\.\., H, W\)"):
            call(torch.zeros(8, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="16384"):
            call(torch.zeros(16385, 1, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="16384"):
            call(torch.zeros(1, 16385, dtype=torch.uint8))
        with pytest.raises(L.OctError, match="no CPU fallback"):   # every other check comes first and needs no device
            call(m)


def _desc(L, images=3, h=130, w=33, classes=9, map_elem=0, has_ignore=1, planes=4, op=0, ignore=255):
    return L.DtDesc(images, h, w, classes, map_elem, has_ignore, planes, op, ignore)


def test_abi_workspace_formula_and_rejected_descriptors(L):
    lib = L.lib()

    def up(v):
        return (v + 255) // 256 * 256

    n, segs = 3 * 130 * 33, 3                              # ceil(130 / 64) segments of a column
    rows, cols = C.c_int(0), C.c_int(0)
    assert lib.oct_dt_block(C.byref(rows), C.byref(cols)) == 0 and rows.value == 64 and cols.value >= 256
    assert lib.oct_dt_block(None, None) == -22
    for op, g in ((L.DT_OP_SQUARED, 4), (L.DT_OP_WEIGHT, 4), (L.DT_OP_SIGNED, 8)):
        want = up(2 * g * n) + up(8 * g * 3 * segs * 33) + up(4 * g * 3)
        assert lib.oct_dt_workspace_bytes(C.byref(_desc(L, op=op))) == want
        assert lib.oct_dt_workspace_bytes(C.byref(_desc(L, op=op, map_elem=2))) == up(n) + want
    plane_list = (C.c_int32 * 8)(0, 0, 1, 0, 2, 8, 1, 3)
    ids = (C.c_int32 * 4)(0, 1, 2, 8)

    def calls(d):
        return (lib.oct_dt_squared(C.byref(d), plane_list, None, None, None, None),
                lib.oct_dt_weight_map(C.byref(d), plane_list, None, None, 1, None, None, None),
                lib.oct_dt_signed(C.byref(d), ids, None, None, None, None))

    bad = ((_desc(L, h=16385), "16384"), (_desc(L, w=16385), "16384"), (_desc(L, classes=17), "classes"),
           (_desc(L, classes=0), "classes"), (_desc(L, map_elem=1), "uint8"), (_desc(L, h=0), "geometry"),
           (_desc(L, images=-1), "geometry"), (_desc(L, op=3), "op"), (_desc(L, planes=0), "empty"),
           (_desc(L, planes=65), "at most 64"), (_desc(L, images=40000, h=16384, w=16384), "2^31"))
    for d, msg in bad:
        assert lib.oct_dt_workspace_bytes(C.byref(d)) == 0 and msg in L.last_error(), msg
        for k in range(3):
            assert calls(d)[k] == -22 and msg in L.last_error(), (msg, k)
    assert lib.oct_dt_workspace_bytes(None) == 0 and "null descriptor" in L.last_error()
    assert lib.oct_dt_workspace_bytes(C.byref(_desc(L, planes=33, op=L.DT_OP_SIGNED))) == 0 and "at most 32" in L.last_error()
    d = _desc(L)
    assert calls(d) == (-22, -22, -22) and "null map" in L.last_error()
    assert lib.oct_dt_squared(C.byref(d), None, None, None, None, None) == -22 and "null plane list" in L.last_error()
    assert lib.oct_dt_signed(C.byref(d), None, None, None, None, None) == -22 and "null class list" in L.last_error()
    assert lib.oct_dt_weight_map(C.byref(d), plane_list, None, None, 0, None, None, None) == -22 and "table is empty" in L.last_error()
    for k, c, msg in ((3, 0, "unknown kind"), (-1, 0, "unknown kind"), (1, 9, "names class"), (2, -1, "names class"),
                      (0, 1, "names class")):
        plane_list[2], plane_list[3] = k, c
        assert lib.oct_dt_squared(C.byref(d), plane_list, None, None, None, None) == -22 and msg in L.last_error(), msg
    ids[1] = 9
    assert lib.oct_dt_signed(C.byref(d), ids, None, None, None, None) == -22 and "names class" in L.last_error()
    ids[1] = 1
    d = _desc(L, images=0)                                 # nothing to do: no pointer is looked at
    plane_list[2], plane_list[3] = 1, 0
    assert calls(d) == (0, 0, 0)
