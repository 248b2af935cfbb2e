"""CPU: the contour-metric restatement (tests/contour_ref.py) and the host formulas evaluation.contour_metrics_from_records on
known answers, the two against each other, the argument errors of BoundaryEvaluator and the two C-ABI symbols.  The ASSD bound
2^-17 px is the derived truncation bound of sum_q = sum floor(2^16 sqrt(D2)) (each term is short by less than 2^-16 in doubled
units, i.e. 2^-17 px, and so is every mean of them); HD95 differs from np.percentile only by the order of the float
interpolation (1e-12 relative)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import contour_ref as R
import eval_ref

ASSD_BOUND = 2.0 ** -17


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


@pytest.mark.parametrize("name", sorted(R.KNOWN))
def test_known_answers(name):
    make, hd, hd95, assd, npts = R.KNOWN[name]
    t, p = make()
    rec = R.mask_records(t, p)
    assert rec.shape == (1, 1, 2, 5) and (rec[0, 0, :, 0] == npts).all()
    m = _E().contour_metrics_from_records(rec)
    assert m["hausdorff"][0, 0] == hd
    assert abs(m["hd95"][0, 0] - hd95) <= 1e-12 * hd95
    assert abs(m["assd"][0, 0] - assd) <= ASSD_BOUND
    assert m["defined"][0, 0] and m["images"] == 1
    f_hd, f_hd95, f_assd = R.float_metrics(1 - t[None].astype(np.int64), 1 - p[None].astype(np.int64), 1)
    assert f_hd[0, 0] == hd and abs(f_hd95[0, 0] - hd95) <= 1e-12 * hd95 and abs(f_assd[0, 0] - assd) <= 1e-12
    assert m["mean_hausdorff"][0] == hd and m["mean_hd95"][0] == m["hd95"][0, 0] and m["mean_assd"][0] == m["assd"][0, 0]


def test_identical_masks_give_zero_and_masks_without_a_contour_nan():
    E = _E()
    t, _ = R.two_rectangles()
    m = E.contour_metrics_from_records(R.mask_records(t, t))
    assert m["hausdorff"][0, 0] == 0.0 and m["hd95"][0, 0] == 0.0 and m["assd"][0, 0] == 0.0
    for flat in (np.zeros((6, 7), dtype=np.uint8), np.ones((6, 7), dtype=np.uint8)):
        assert len(R.contour_points(flat != 0)) == 0
        for a, b in ((flat, flat), (flat, t[:6, :7]), (t[:6, :7], flat)):
            rec = R.mask_records(a, b)
            assert (rec[..., 1:] == 0).all()
            m = E.contour_metrics_from_records(rec)
            assert not m["defined"][0, 0]
            assert np.isnan(m["hausdorff"][0, 0]) and np.isnan(m["hd95"][0, 0]) and np.isnan(m["assd"][0, 0])
            assert np.isnan(m["mean_hausdorff"][0]) and np.isnan(m["mean_hd95"][0]) and np.isnan(m["mean_assd"][0])


def test_points_of_a_single_pixel_and_of_the_ignored_neighbourhood():
    m = np.zeros((5, 6), dtype=bool)
    m[2, 3] = True
    assert sorted(map(tuple, R.contour_points(m))) == [(3, 6), (4, 5), (4, 7), (5, 6)]
    out = np.zeros((5, 6), dtype=bool)
    out[2, 4] = True                                      # the right neighbour is outside the image: that pair yields no point
    assert sorted(map(tuple, R.contour_points(m, out))) == [(3, 6), (4, 5), (5, 6)]
    corner = np.zeros((3, 3), dtype=bool)
    corner[0, 0] = True                                   # nothing along the image border
    assert sorted(map(tuple, R.contour_points(corner))) == [(0, 1), (1, 0)]


@pytest.mark.parametrize("kind,classes,ignore", [("layered", 9, None), ("layered", 9, 255), ("random", 3, None)])
def test_host_formulas_agree_with_the_percentile_path(kind, classes, ignore):
    rng = np.random.default_rng(11)
    shape = (2, 33, 130) if kind == "layered" else (2, 12, 17)
    t, p = (eval_ref.layered_maps if kind == "layered" else eval_ref.random_maps)(rng, shape, classes)
    if ignore is not None:
        t = t.copy()
        t[rng.random(shape) < 0.25] = ignore
    m = _E().contour_metrics_from_records(R.records(t, p, classes, ignore))
    hd, hd95, assd = R.float_metrics(t, p, classes, ignore)
    d = m["defined"]
    assert d.any() and (np.isnan(hd) == ~d).all()
    assert (m["hausdorff"][d] == hd[d]).all()
    assert (np.abs(m["hd95"][d] - hd95[d]) <= 1e-12 * hd95[d]).all()
    assert (np.abs(m["assd"][d] - assd[d]) <= ASSD_BOUND).all() and (m["assd"][d] <= assd[d] + 1e-12).all()
    for k in ("hausdorff", "hd95", "assd"):
        assert np.isnan(m[k][~d]).all()
        for c in range(classes):
            want = m[k][d[:, c], c].mean() if d[:, c].any() else np.nan
            assert m["mean_" + k][c] == want or (np.isnan(want) and np.isnan(m["mean_" + k][c]))


def test_layered_fixture_has_every_contour_on_both_sides():
    """the GPU test relies on it"""
    t, p = eval_ref.layered_maps(np.random.default_rng(0), (2, 33, 130), 9)
    rec = R.records(t, p, 9)
    assert (rec[..., 0] > 0).all() and _E().contour_metrics_from_records(rec)["defined"].all()


def test_records_shape_is_checked():
    E = _E()
    with pytest.raises(ValueError, match="records"):
        E.contour_metrics_from_records(np.zeros((2, 3, 2, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="records"):
        E.contour_metrics_from_records(np.zeros((2, 3, 2, 5), dtype=np.float64))
    m = E.contour_metrics_from_records(np.zeros((0, 3, 2, 5), dtype=np.int64))
    assert m["images"] == 0 and m["hausdorff"].shape == (0, 3) and np.isnan(m["mean_assd"]).all()


def test_boundary_evaluator_argument_errors(L):
    E = _E()
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="classes"):
            E.BoundaryEvaluator(bad)
    with pytest.raises(TypeError, match="classes"):
        E.BoundaryEvaluator(2.0)
    with pytest.raises(TypeError, match="ignore_index"):
        E.BoundaryEvaluator(2, ignore_index=1.5)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        E.BoundaryEvaluator(2, max_workspace_bytes=0)
    with pytest.raises(L.OctError, match="GPU"):
        E.BoundaryEvaluator(2, device="cpu")
    ev = E.BoundaryEvaluator(3)
    z = torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(TypeError, match="integer class map"):
        ev.update(z.float(), z)
    with pytest.raises(TypeError, match="integer class map"):
        ev.update(z, z.double())
    with pytest.raises(TypeError, match="torch tensor"):
        ev.update(z.numpy(), z)
    with pytest.raises(RuntimeError, match="same shape"):
        ev.update(z, z[:, :, :4])
    with pytest.raises(RuntimeError, match=r"\(\.\.\., H, W\)"):
        ev.update(z[0, 0], z[0, 0])
    with pytest.raises(L.OctError, match="no CPU fallback"):
        ev.update(z, z)
    tall = torch.zeros(1, 16385, 1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="16384"):
        ev.update(tall, tall)
    with pytest.raises(RuntimeError, match="16384"):
        ev.update(tall.reshape(1, 1, 16385), tall.reshape(1, 1, 16385))
    with pytest.raises(ValueError, match="records"):
        ev.merge(np.zeros((1, 2, 2, 5), dtype=np.int64))
    with pytest.raises(TypeError, match="update"):
        ev.update_model(torch.nn.Conv2d(1, 3, 1), z, z)
    assert ev.records().shape == (0, 3, 2, 5) and ev.compute()["images"] == 0


def test_merge_and_compute_need_no_gpu():
    E = _E()
    t, p = R.two_pixels()
    rec = R.mask_records(t, p)
    ev = E.BoundaryEvaluator(1).merge(rec).merge(torch.from_numpy(rec))
    m = ev.compute()
    assert m["images"] == 2 and (m["hausdorff"] == 3.0).all()
    assert ev.reset().compute()["images"] == 0


def test_abi_symbols_load_and_validate_without_a_gpu(L):
    lib = L.lib()
    d = L.ContourDesc(3, 33, 130, 9, 0, 2, 1, 255)
    hd, wd = 65, 259
    s = hd * wd

    def up(v):
        return (v + 255) // 256 * 256

    want = (up(2 * 3 * 33 * 130) + up(4 * 3 * 9 * s) + up(16 * 3 * 9 * 2 * wd) + up(16 * 3 * (s // 2)) + up(8 * 3 * 9) + up(32 * 3 * 9)
            + up(4096 * 3 * 9))                          # the header's formula; 65 site rows are two segments of 64
    assert lib.oct_contour_workspace_bytes(C.byref(d)) == want
    one = lib.oct_contour_workspace_bytes(C.byref(L.ContourDesc(1, 33, 130, 9, 0, 2, 1, 255)))
    assert 0 < one and 3 * one >= want                    # the chunking rule: bytes(k) <= k * bytes(1)
    for bad, msg in ((L.ContourDesc(1, 16385, 4, 2, 0, 0, 0, 0), "16384"), (L.ContourDesc(1, 4, 4, 17, 0, 0, 0, 0), "classes"),
                     (L.ContourDesc(1, 4, 4, 2, 1, 0, 0, 0), "uint8"), (L.ContourDesc(1, 0, 4, 2, 0, 0, 0, 0), "geometry")):
        assert lib.oct_contour_workspace_bytes(C.byref(bad)) == 0 and msg in L.last_error()
        assert lib.oct_contour_update(C.byref(bad), None, None, None, None, None) == -22 and msg in L.last_error()
    assert lib.oct_contour_update(None, None, None, None, None, None) == -22 and "null descriptor" in L.last_error()
    assert lib.oct_contour_update(C.byref(d), None, None, None, None, None) == -22 and "null input" in L.last_error()
