"""GPU: the contour metrics (csrc/contour.hip, evaluation.BoundaryEvaluator, Metrics.Contour_based_metrics) against the integer
restatement tests/contour_ref.py.  Every comparison of records is == on int64, over the whole record tensor: the undefined
cases (n and zeros) are compared like the others.  Shapes are the smallest at which the kernels can go wrong: no site, one
site, odd tails, a doubled width of 259 (two 256-thread column strips, five 64-lane waves), more rows than one block of
sites, leading dimensions, a walk over the full row length, a misaligned view."""
import functools

import numpy as np
import pytest
import torch

import contour_ref as R
import eval_ref
from oracle.bounds import Out, seed

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 5, 7), (3, 33, 130), (1, 70, 64), (2, 3, 4, 40)]
CLASSES = [1, 2, 9, 16]
KINDS = ("layered", "random", "one_class")
DTYPES = {"u8": torch.uint8, "i64": torch.int64}
# target dtype, pred dtype, ignore_index
COMBOS = [("u8", "u8", None), ("u8", "i64", 255), ("i64", "u8", -100), ("i64", "i64", None)]


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


@functools.lru_cache(maxsize=None)
def _maps(shape, classes, kind, ignore):
    """(target, pred, reference records): computed once per case, never modified.  The ignored pixels do not depend on the
    value that marks them, so 255 and -100 share one reference."""
    if ignore not in (None, 255):
        t, p, ref = _maps(shape, classes, kind, 255)
        t = np.where(t == 255, ignore, t)
        t.setflags(write=False)
        return t, p, ref
    rng = np.random.default_rng(seed(shape, classes, kind, ignore))
    if kind == "layered":
        t, p = eval_ref.layered_maps(rng, shape, classes)
    elif kind == "random":
        t, p = eval_ref.random_maps(rng, shape, classes)
    else:   # one label everywhere: no contour anywhere
        t = np.full(shape, classes - 1, dtype=np.int64)
        p = t.copy()
    if ignore is not None:
        t = t.copy()
        t[rng.random(shape) < 0.25] = ignore
    t.setflags(write=False)
    p.setflags(write=False)
    ref = R.records(t, p, classes, ignore)
    ref.setflags(write=False)
    return t, p, ref


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _records(ev):
    return ev.records().cpu().numpy()


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_records_match_the_restatement(shape, classes):
    E = _E()
    images = int(np.prod(shape[:-2]))
    for kind in KINDS:
        for tn, pn, ignore in COMBOS:
            t, p, ref = _maps(shape, classes, kind, ignore)
            ev = E.BoundaryEvaluator(classes, ignore_index=ignore).update(_dev(t, DTYPES[tn]), _dev(p, DTYPES[pn]))
            got = _records(ev)
            print(shape, classes, kind, tn, pn, ignore, "points", got[..., 0].sum(), "max d2", got[..., 1].max())
            assert got.shape == (images, classes, 2, 5)
            np.testing.assert_array_equal(got, ref, err_msg=f"{kind} target {tn} pred {pn} ignore {ignore}")
            if kind == "one_class":
                assert not got.any()
    m = ev.compute()
    assert m["images"] == images and m["hausdorff"].shape == (images, classes)


def test_the_layered_case_is_defined_everywhere_and_the_metrics_follow_the_float_path():
    E = _E()
    t, p = eval_ref.layered_maps(np.random.default_rng(0), (2, 33, 130), 9)
    ev = E.BoundaryEvaluator(9).update(_dev(t, torch.uint8), _dev(p, torch.uint8))
    np.testing.assert_array_equal(_records(ev), R.records(t, p, 9))
    m = ev.compute()
    hd, hd95, assd = R.float_metrics(t, p, 9)
    assert m["defined"].all()
    assert (m["hausdorff"] == hd).all()
    assert (np.abs(m["hd95"] - hd95) <= 1e-12 * hd95).all()
    assert (np.abs(m["assd"] - assd) <= 2.0 ** -17).all()
    assert (m["mean_hausdorff"] == m["hausdorff"].mean(axis=0)).all()


def test_far_corners_walk_the_full_row():
    """one pixel in opposite corners of target and pred: the nearest point lies a whole row length away"""
    E = _E()
    t, p = np.ones((1, 40, 200), dtype=np.int64), np.ones((1, 40, 200), dtype=np.int64)
    t[0, 0, 0] = 0
    p[0, 39, 199] = 0
    ref = R.records(t, p, 2)
    assert (ref[..., 0] == 2).all() and ref[..., 1].max() == 77 ** 2 + 397 ** 2
    for tdt, pdt in ((torch.uint8, torch.int64), (torch.int64, torch.uint8)):
        np.testing.assert_array_equal(_records(E.BoundaryEvaluator(2).update(_dev(t, tdt), _dev(p, pdt))), ref)
    # the same down a tall image: 399 site rows are seven 64-row segments of a column, five of them without a point
    t, p = np.ones((1, 200, 3), dtype=np.int64), np.ones((1, 200, 3), dtype=np.int64)
    t[0, 0, 1] = 0
    p[0, 199, 1] = 0
    ref = R.records(t, p, 2)
    assert (ref[..., 0] == 3).all() and ref[..., 1].max() == 397 ** 2 + 1
    np.testing.assert_array_equal(_records(E.BoundaryEvaluator(2).update(_dev(t, torch.uint8), _dev(p, torch.uint8))), ref)
    # one row of 2100 pixels: D2 = 4196^2 > 2^24, the only case here whose D2 reaches the top byte of the radix select
    t, p = np.ones((1, 1, 2100), dtype=np.int64), np.ones((1, 1, 2100), dtype=np.int64)
    t[0, 0, 0] = 0
    p[0, 0, 2099] = 0
    ref = R.records(t, p, 2)
    assert (ref[..., 0] == 1).all() and (ref[..., 1:4] == 4196 ** 2).all() and 4196 ** 2 > 2 ** 24
    np.testing.assert_array_equal(_records(E.BoundaryEvaluator(2).update(_dev(t, torch.uint8), _dev(p, torch.int64))), ref)


def test_labels_outside_the_classes_belong_to_no_class():
    E = _E()
    rng = np.random.default_rng(seed("outside"))
    t, p = rng.integers(0, 5, size=(2, 9, 70)), rng.integers(0, 5, size=(2, 9, 70))
    bad = [-1, -2 ** 63, 2 ** 63 - 1, 2 ** 40, 256 + 1, 3]
    for a in (t, p):
        mask = rng.random(a.shape) < 0.1
        a[mask] = rng.choice(bad, size=int(mask.sum()))
    ref = R.records(t, p, 3)
    np.testing.assert_array_equal(_records(E.BoundaryEvaluator(3).update(_dev(t, torch.int64), _dev(p, torch.int64))), ref)
    t8, p8 = (t % 256).astype(np.uint8), (p % 256).astype(np.uint8)
    np.testing.assert_array_equal(_records(E.BoundaryEvaluator(3).update(_dev(t8, torch.uint8), _dev(p8, torch.uint8))),
                                  R.records(t8, p8, 3))


def _left_band(shape, rows, width):
    """a rectangle on the left border: 2 * width + rows points (nothing along the border)"""
    m = np.ones(shape, dtype=np.int64)
    m[2:2 + rows, :width] = 0
    return m


def _selection_cases():
    pixel = np.ones((6, 30), dtype=np.int64)
    pixel[4, 17] = 0
    one = np.ones((1, 2), dtype=np.int64)
    one[0, 0] = 0                                         # n = 1
    two = np.ones((1, 3), dtype=np.int64)
    two[0, 1] = 0                                         # n = 2
    two_b = np.ones((1, 3), dtype=np.int64)
    two_b[0, 0] = 0                                       # n = 1 against n = 2
    band_t = (np.arange(12)[:, None] >= 4).astype(np.int64) * np.ones((1, 9), dtype=np.int64)
    band_p = (np.arange(12)[:, None] >= 7).astype(np.int64) * np.ones((1, 9), dtype=np.int64)
    empty = np.ones((6, 30), dtype=np.int64)
    return {
        "n1": (one, one.copy(), 1), "n2": (two, two_b, 2),
        "n21": (_left_band((6, 30), 1, 10), pixel, 21), "n41": (_left_band((6, 30), 1, 20), pixel, 41),
        "translate": (band_t, band_p, 9),                 # a full-width boundary moved by 3 rows: every D2 is 36
        "no_contour_in_pred": (pixel, empty, 4), "no_contour_in_target": (empty, pixel, 0),
    }


@pytest.mark.parametrize("name", sorted(_selection_cases()))
def test_selection_edge_cases(name):
    E = _E()
    t, p, n_target = _selection_cases()[name]
    ref = R.records(t[None], p[None], 2)
    assert ref[0, 0, 1, 0] == n_target                    # direction 1: the points of target
    if name in ("n21", "n41"):
        assert (19 * (n_target - 1)) % 20 == 0
    if name == "translate":
        assert (ref[0, :, :, 1:4] == 36).all()
    for tdt in (torch.uint8, torch.int64):
        got = _records(E.BoundaryEvaluator(2).update(_dev(t[None], tdt), _dev(p[None], torch.int64)))
        np.testing.assert_array_equal(got, ref, err_msg=name)
        rev = _records(E.BoundaryEvaluator(2).update(_dev(p[None], tdt), _dev(t[None], torch.int64)))
        np.testing.assert_array_equal(rev, ref[:, :, ::-1], err_msg=name + " reversed")
    m = E.contour_metrics_from_records(got)
    assert m["defined"].all() == (not name.startswith("no_contour"))


@pytest.mark.parametrize("which", ["target", "pred", "both"])
def test_misaligned_uint8_views(which):
    """maps[1:] of a 5 x 7 uint8 batch starts 35 bytes into its storage"""
    E = _E()
    t, p, ref = _maps((4, 5, 7), 3, "random", None)
    dt, dp = _dev(t, torch.uint8), _dev(p, torch.uint8)
    vt = dt[1:] if which in ("target", "both") else dt[1:].clone()
    vp = dp[1:] if which in ("pred", "both") else dp[1:].clone()
    assert (vt.data_ptr() % 16 != 0 or which == "pred") and (vp.data_ptr() % 16 != 0 or which == "target")
    np.testing.assert_array_equal(_records(E.BoundaryEvaluator(3).update(vt, vp)), ref[1:])


def test_chunks_updates_and_repeats_give_the_same_bits_without_a_synchronisation():
    E = _E()
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    import ctypes as C
    shape, classes = (3, 33, 130), 9
    t, p, ref = _maps(shape, classes, "layered", 255)
    dt, dp = _dev(t, torch.uint8), _dev(p, torch.int64)
    one = L.lib().oct_contour_workspace_bytes(C.byref(L.ContourDesc(1, 33, 130, classes, 0, 2, 1, 255)))
    whole = E.BoundaryEvaluator(classes, ignore_index=255)
    chunked = E.BoundaryEvaluator(classes, ignore_index=255, max_workspace_bytes=one)   # one image per launch: three chunks
    split = E.BoundaryEvaluator(classes, ignore_index=255)
    whole.update(dt, dp)                                  # loads the library, allocates: before the sync check
    chunked.update(dt, dp).reset()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        chunked.update(dt, dp)
        split.update(dt[:1], dp[:1]).update(dt[1:], dp[1:])
        whole.update(dt, dp)                              # the same update again
        recs = [whole.records(), chunked.records(), split.records()]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert chunked._workspace.numel() == one and whole._workspace.numel() > 2 * one
    w, c, s = (r.cpu().numpy() for r in recs)
    np.testing.assert_array_equal(c, ref)
    np.testing.assert_array_equal(s, ref)
    np.testing.assert_array_equal(w, np.concatenate([ref, ref]))
    with pytest.raises(RuntimeError, match="max_workspace_bytes"):
        E.BoundaryEvaluator(classes, max_workspace_bytes=one - 1).update(dt, dp)
    merged = E.BoundaryEvaluator(classes).merge(split.records()[:1]).merge(split.records()[1:].cpu().numpy())
    np.testing.assert_array_equal(_records(merged), ref)
    assert whole.reset().compute()["images"] == 0


def test_records_are_written_inside_their_buffer_only():
    """the raw entry point with a sentinel-tailed records buffer and a workspace of exactly the size asked for"""
    import ctypes as C
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    t, p, ref = _maps((3, 33, 130), 9, "layered", None)
    dt, dp = _dev(t, torch.int64), _dev(p, torch.int64)
    desc = L.ContourDesc(3, 33, 130, 9, 2, 2, 0, 0)
    need = L.lib().oct_contour_workspace_bytes(C.byref(desc))
    ws = Out((need,), torch.uint8, fill=0x5A)
    out = Out((3, 9, 2, 5), torch.int64, fill=-7777)
    L.check(L.lib().oct_contour_update(C.byref(desc), dt.data_ptr(), dp.data_ptr(), out.ptr(), ws.ptr(),
                                       torch.cuda.current_stream().cuda_stream), "oct_contour_update")
    np.testing.assert_array_equal(out.host(), ref)
    ws.host()                                             # asserts the sentinel tail of the workspace


@pytest.mark.parametrize("name", sorted(R.KNOWN))
def test_metric_functions_on_the_known_answers(name):
    from retinal_oct_image_segmentation_via_deep_learning_amd.Metrics import Contour_based_metrics as M
    make, hd, hd95, assd, _ = R.KNOWN[name]
    t, p = make()
    want = _E().contour_metrics_from_records(R.mask_records(t, p))
    forms = {"numpy": (t, p), "bool": (t.astype(bool), p.astype(bool)), "float": (t.astype(np.float32), p * 0.75),
             "device": (torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda()), "mixed": (t, torch.from_numpy(p).cuda().long())}
    for form, (a, b) in forms.items():
        got = M.hausdorff_distance(a, b), M.hausdorff_distance_95(a, b), M.assd(a, b)
        assert all(type(v) is np.float64 for v in got), form
        assert got[0] == hd, form
        assert abs(got[1] - hd95) <= 1e-12 * hd95 and abs(got[2] - assd) <= 2.0 ** -17, form
        assert got == (want["hausdorff"][0, 0], want["hd95"][0, 0], want["assd"][0, 0]), form
    assert M.hausdorff_distance(t, t) == 0.0 and M.hausdorff_distance_95(t, t) == 0.0 and M.assd(t, t) == 0.0
    for flat in (np.zeros_like(t), np.ones_like(t)):
        assert np.isnan(M.hausdorff_distance(t, flat)) and np.isnan(M.hausdorff_distance_95(flat, t)) and np.isnan(M.assd(flat, flat))
    with pytest.raises(ValueError, match="2-D"):
        M.hausdorff_distance(t[None], p[None])
    with pytest.raises(ValueError, match="2-D"):
        M.assd(t[0], p[0])


def test_mad_equals_the_mean_squared_error_on_masks():
    from retinal_oct_image_segmentation_via_deep_learning_amd.Metrics import Contour_based_metrics as M
    from retinal_oct_image_segmentation_via_deep_learning_amd.Metrics import PixelError_based_metrics as P
    rng = np.random.default_rng(8)
    t, p = rng.integers(0, 2, size=(37, 53)), rng.integers(0, 2, size=(37, 53))
    want = np.mean(np.abs(t.astype(float) - p.astype(float)))
    for a, b in ((t, p), (t.astype(np.uint8), p.astype(bool)), (t.astype(np.float32), p.astype(np.float32)),
                 (torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())):
        got = M.mad(a, b)
        assert type(got) is np.float64 and got == want and got == P.mean_squared_error(a, b)
    f, g = rng.random((5, 9)).astype(np.float32), rng.random((5, 9))
    # two float64 sums of 45 terms below 1 in different orders: each within 44 * 2^-53 * 45 of the exact sum, then / 45
    assert abs(M.mad(f, g) - np.mean(np.abs(f.astype(float) - g))) <= 2 * 44 * 2.0 ** -53


def test_update_model_equals_update_on_predict():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as MG
    E = _E()
    torch.manual_seed(3)
    model = UNet(1, 8, init_features=4).cuda().eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 32, 32, generator=g).cuda()
    t = torch.randint(0, 8, (2, 32, 32), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.1] = 255
    t = t.to(torch.uint8).cuda()
    a = E.BoundaryEvaluator(8, ignore_index=255).update_model(model, x, t)
    pred = model.predict(x)
    b = E.BoundaryEvaluator(8, ignore_index=255).update(t, pred)
    np.testing.assert_array_equal(_records(a), _records(b))
    np.testing.assert_array_equal(_records(a), R.records(t.cpu().numpy(), pred.cpu().numpy(), 8, 255))
    with pytest.raises(TypeError, match="update"):
        E.BoundaryEvaluator(3).update_model(MG.MGUNet_2(1, 3, feature_scale=16), x, t)
