"""GPU: the distance maps (csrc/distance.hip, distance.py) against the numpy restatement tests/dt_ref.py.  Squared distances and
table-mapped weights are compared with == on whole tensors.  The shapes come from oct_dt_block = (R, Cw), the rows of a
column-pass unit and the pixels of a row-pass workgroup, so they keep straddling both if either changes: one pixel, one row over
three workgroups, one column over three units, exactly one unit by one workgroup, one more each way, three each way with ragged
edges, and the two limits (1, 16384) -- the longest row LDS holds -- and (16384, 1) -- the largest column distance uint16 holds.
The patterns: no site, every pixel a site, one site in each corner (the longest walk), sites in the first and last column only,
1 % and 50 % noise, a checkerboard, 2-, 3- and 9-class noise, wavy bands of six classes (what an OCT map looks like), an ignored
rectangle, an ignored frame (what the augmenter leaves), labels out of range."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dt_ref as R
from oracle.bounds import Out, seed

pytestmark = pytest.mark.gpu

SHAPE_NAMES = ("pixel", "row", "column", "block", "block_plus_one", "three_blocks", "longest_row", "longest_column")
PATTERNS = ("no_site", "all_sites", "corner_tl", "corner_tr", "corner_bl", "corner_br", "edge_columns", "noise_1pct", "noise_50pct",
            "checkerboard", "noise2", "noise3", "noise9", "bands6", "ignored_rectangle", "ignored_frame", "out_of_range_u8",
            "out_of_range_i64")
IGNORE = 7


def _D():
    from retinal_oct_image_segmentation_via_deep_learning_amd import distance
    return distance


def _L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _shape(name):
    r, cw = _D().block()
    return {"pixel": (1, 1), "row": (1, 2 * cw + 3), "column": (2 * r + 3, 1), "block": (r, cw), "block_plus_one": (r + 1, cw + 1),
            "three_blocks": (2 * r + 3, 2 * cw + 5), "longest_row": (1, 16384), "longest_column": (16384, 1)}[name]


@functools.lru_cache(maxsize=None)
def _pattern(name, shape_name):
    """(int64 map [1, h, w], classes, ignore_index, fits uint8, planes), read-only"""
    h, w = _shape(shape_name)
    rng = np.random.default_rng(seed(name, shape_name))
    classes, ignore, u8 = 2, None, True
    planes = ["boundary", ("class", 1), ("other", 1)]
    m = np.zeros((1, h, w), dtype=np.int64)
    if name == "no_site":                                  # one class everywhere: no boundary, no class 1, nothing but class 0
        planes = ["boundary", ("class", 1), ("other", 0)]
    elif name == "all_sites":
        planes = [("class", 0), ("other", 1)]
    elif name.startswith("corner_"):
        m[0, 0 if name[7] == "t" else h - 1, 0 if name[8] == "l" else w - 1] = 1
        planes = [("class", 1), "boundary"]
    elif name == "edge_columns":
        m[:, :, 0] = m[:, :, w - 1] = 1
        planes = [("class", 1)]
    elif name in ("noise_1pct", "noise_50pct"):
        m = (rng.random((1, h, w)) < (0.01 if name == "noise_1pct" else 0.5)).astype(np.int64)
    elif name == "checkerboard":
        m = ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1)[None].astype(np.int64)
    elif name in ("noise2", "noise3", "noise9"):
        classes = int(name[5:])
        m = rng.integers(0, classes, size=(1, h, w))
        planes = ["boundary"]
    elif name == "bands6":                                 # nine classes declared: 6, 7 and 8 are absent
        classes = 9
        m = R.wavy_bands(rng, (1, h, w), 6)
        planes = ["boundary", ("class", 0), ("class", 3), ("other", 5), ("class", 7), ("other", 8)]
    elif name in ("ignored_rectangle", "ignored_frame"):
        classes, ignore = 9, IGNORE
        m = R.wavy_bands(rng, (1, h, w), 6)
        if name == "ignored_rectangle":
            m[:, h // 4:h // 4 + max(1, h // 3), w // 5:w // 5 + max(1, w // 2)] = IGNORE
        else:                                              # the frame a rotated crop leaves around the labels
            fy, fx = min(5, h // 3), min(9, w // 3)
            frame = np.ones((h, w), dtype=bool)
            frame[fy:h - fy, fx:w - fx] = False
            m[:, frame] = IGNORE
        planes = ["boundary", ("class", 2), ("other", 2)]
    elif name == "out_of_range_u8":
        classes, ignore = 3, 1
        m = rng.integers(0, 3, size=(1, h, w))
        m[rng.random(m.shape) < 0.2] = 200
        planes = ["boundary", ("class", 2), ("other", 2), ("class", 1)]
    else:
        classes, u8 = 3, False
        m = rng.integers(0, 3, size=(1, h, w))
        r = rng.random(m.shape)
        m[r < 0.15] = -5
        m[r > 0.85] = 2 ** 40 + 1                          # its low byte is a class: the narrowing must look at all 64 bits
        planes = ["boundary", ("class", 1), ("other", 1)]
    m = m.astype(np.int64)
    m.setflags(write=False)
    return m, classes, ignore, u8, tuple(planes)


@functools.lru_cache(maxsize=None)
def _ref(name, shape_name):
    m, classes, ignore, _, planes = _pattern(name, shape_name)
    d2 = R.squared_distance(m, classes, list(planes), ignore)
    d2.setflags(write=False)
    return d2


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()   # a copy: the cached cases are read-only


def _offset_by_one(t):
    """the same values in a buffer whose base is one element past an aligned allocation"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_squared_distance_equals_the_restatement(shape_name, name):
    D = _D()
    m, classes, ignore, u8, planes = _pattern(name, shape_name)
    want = _ref(name, shape_name)
    got = []
    for dtype in ((torch.uint8, torch.int64, torch.int32) if u8 else (torch.int64,)):
        for shift in (False, True):
            x = _dev(m, dtype)
            x = _offset_by_one(x) if shift else x
            d2 = D.squared_distance(x, classes, list(planes), ignore)
            again = D.squared_distance(x, classes, list(planes), ignore)
            assert d2.dtype == torch.int32 and d2.shape == (1, len(planes)) + x.shape[-2:] and d2.is_contiguous()
            assert torch.equal(d2, again), f"{name}: two runs differ"
            got.append(d2.cpu().numpy())
    finite = want[want < R.FAR]
    print(shape_name, name, "largest D2", int(finite.max()) if finite.size else None, "planes without a site",
          int((want.reshape(len(planes), -1)[:, 0] == R.FAR).sum()))
    for d2 in got:                                         # uint8, int64 and int32, aligned and offset: all the same bits
        np.testing.assert_array_equal(d2, want, err_msg=name)
    h, w = m.shape[-2:]
    if name == "no_site":
        assert (got[0] == R.FAR).all() and R.FAR == D.FAR == 1 << 30
    if name == "all_sites":
        assert not got[0].any()
    if name == "corner_br":                                # the known answer, whatever the restatement says
        yy, xx = np.mgrid[0:h, 0:w]
        np.testing.assert_array_equal(got[0][0, 0], (h - 1 - yy) ** 2 + (w - 1 - xx) ** 2)


def test_three_images_and_all_plane_kinds_in_one_call():
    """different contents per image (the image strides), every plane kind, the class present in some images and absent in
    others, leading dimensions kept"""
    D = _D()
    h, w = _shape("block_plus_one")
    rng = np.random.default_rng(seed("three images"))
    m = np.stack([R.wavy_bands(rng, (h, w), 6), rng.integers(0, 3, size=(h, w)), np.full((h, w), 4)]).astype(np.int64)
    m[1][rng.random((h, w)) < 0.1] = 255
    planes = ["boundary", ("class", 1), ("other", 1), ("class", 4), ("other", 4), ("class", 8), ("other", 8)]
    want = R.squared_distance(m, 9, planes, 255)
    assert (want[2, 0] == R.FAR).all() and (want[1, 3] == R.FAR).all() and not want[2, 3].any() and (want[0, 5] == R.FAR).all()
    for dtype in (torch.uint8, torch.int64):
        got = D.squared_distance(_dev(m, dtype), 9, planes, 255)
        assert got.shape == (3, 7, h, w)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        lead = D.squared_distance(_dev(m, dtype).view(3, 1, h, w), 9, planes, 255)
        assert lead.shape == (3, 1, 7, h, w) and torch.equal(lead.view(3, 7, h, w), got)
    empty = D.squared_distance(torch.zeros(0, h, w, dtype=torch.uint8, device="cuda"), 9, planes)
    assert empty.shape == (0, 7, h, w) and empty.dtype == torch.int32


@pytest.mark.parametrize("op", ["squared", "weight", "signed"])
def test_outputs_and_workspace_are_written_inside_their_buffers_only(op):
    """the raw entry points with sentinel-tailed outputs and a sentinel-tailed workspace of exactly the size asked for"""
    L = _L()
    h, w = 67, 131
    rng = np.random.default_rng(seed("canary", op))
    m = np.stack([R.wavy_bands(rng, (h, w), 6), rng.integers(0, 9, size=(h, w)), np.zeros((h, w), dtype=np.int64)])
    stream = torch.cuda.current_stream().cuda_stream
    for elem, dtype in ((0, torch.uint8), (2, torch.int64)):
        x = _dev(m, dtype)
        nplanes = {"squared": 3, "weight": 2, "signed": 4}[op]
        desc = L.DtDesc(3, h, w, 9, elem, 1, nplanes, {"squared": 0, "weight": 1, "signed": 2}[op], 5)
        need = L.lib().oct_dt_workspace_bytes(C.byref(desc))
        assert need > 0
        ws = Out((need,), torch.uint8, fill=0x5A)
        if op == "squared":
            planes = ["boundary", ("class", 2), ("other", 8)]
            out = Out((3, 3, h, w), torch.int32, fill=-7777)
            L.check(L.lib().oct_dt_squared(C.byref(desc), (C.c_int32 * 6)(0, 0, 1, 2, 2, 8), x.data_ptr(), out.ptr(), ws.ptr(), stream))
            np.testing.assert_array_equal(out.host(), R.squared_distance(m, 9, planes, 5))
        elif op == "weight":
            table = np.array([4.0, 3.0, 2.5, 2.0, 1.0], dtype=np.float32)
            out = Out((3, 2, h, w), torch.float32)
            dtable = torch.from_numpy(table).cuda()        # named: it lives until the call has run
            L.check(L.lib().oct_dt_weight_map(C.byref(desc), (C.c_int32 * 4)(0, 0, 1, 3), x.data_ptr(), dtable.data_ptr(), 5, out.ptr(),
                                              ws.ptr(), stream))
            want = R.table_lookup(R.squared_distance(m, 9, ["boundary", ("class", 3)], 5), table)
            np.testing.assert_array_equal(out.host(), want.astype(np.float64))
        else:
            out = Out((3, 4, h, w), torch.float32)
            L.check(L.lib().oct_dt_signed(C.byref(desc), (C.c_int32 * 4)(0, 3, 8, 3), x.data_ptr(), out.ptr(), ws.ptr(), stream))
            want = R.signed_distance(m, 9, [0, 3, 8, 3], 5)
            assert (np.abs(out.host() - want) <= 2.0 ** -23 * np.abs(want)).all()
        ws.host()                                          # asserts the sentinel tail of the workspace


# ---- the weight map --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_name", ["row", "block_plus_one", "three_blocks"])
def test_weight_map_is_the_table_entry_bit_for_bit(shape_name):
    D = _D()
    makers = {"gaussian": lambda ign: D.DistanceWeightMap.gaussian(9, 10.0, 5.0, ignore_index=ign),
              "gaussian_narrow": lambda ign: D.DistanceWeightMap.gaussian(9, 0.3, 0.7, base=0.25, cutoff_sigmas=2.0, ignore_index=ign),
              "boundary_bonus": lambda ign: D.DistanceWeightMap.boundary_bonus(9, 2.0, ignore_index=ign),
              "one_entry": lambda ign: D.DistanceWeightMap(9, [0.75], ignore_index=ign)}
    for name in ("bands6", "ignored_frame", "no_site", "noise_1pct"):
        m, _, ignore, _, planes = _pattern(name, shape_name)
        d2 = _ref(name, shape_name)[:, planes.index("boundary")]
        for maker in makers.values():
            wm = maker(ignore)
            table = wm.table.numpy()
            want = R.table_lookup(d2, table)
            assert want.dtype == np.float32
            for dtype in (torch.uint8, torch.int64):
                x = _dev(m, dtype)
                got = wm(x)
                assert got.dtype == torch.float32 and got.shape == x.shape and got.is_contiguous() and got.device == x.device
                np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=name)   # the bits
            first = wm._workspace
            assert torch.equal(wm(x), got) and wm._workspace is first   # the cached workspace, the same bits
    m, _, ignore, _, _ = _pattern("bands6", shape_name)
    plain = D.DistanceWeightMap.gaussian(9, 10.0, 5.0)(_dev(m)[0])       # (H, W) in, (H, W) out
    assert plain.shape == m.shape[-2:]


# ---- the signed map --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_name", ["pixel", "row", "column", "block_plus_one", "three_blocks"])
def test_signed_distance_is_within_one_ulp_of_float64(shape_name):
    """|err| <= 2^-23 |ref|: D2 is an exact integer, its conversion to fp32 is exact below 2^24 and sqrtf is within an ulp.  The
    shapes keep every distance below 4096 (h, w <= 2053 < 4096 / sqrt(2)), so D2 < 2^24."""
    D = _D()
    h, w = _shape(shape_name)
    assert h * h + w * w < 4096 * 4096
    for name in ("bands6", "ignored_rectangle", "noise3", "corner_tl", "no_site", "out_of_range_i64"):
        m, classes, ignore, u8, _ = _pattern(name, shape_name)
        ids = [0, classes - 1, 1 % classes]
        want = R.signed_distance(m, classes, ids, ignore)
        for dtype in ((torch.uint8, torch.int64) if u8 else (torch.int64,)):
            x = _dev(m, dtype)
            got = D.signed_distance(x, classes, ids, ignore)
            assert got.dtype == torch.float32 and got.shape == (1, 3, h, w) and got.is_contiguous()
            assert torch.equal(got, D.signed_distance(x, classes, ids, ignore)), "two runs differ"
            g = got.cpu().numpy().astype(np.float64)
            err = np.abs(g - want)
            print(shape_name, name, "largest |ref|", float(np.abs(want).max()), "largest err / |ref| in units of 2^-23",
                  float((err[want != 0] / np.abs(want[want != 0])).max() * 2 ** 23) if (want != 0).any() else 0.0)
            assert (err <= 2.0 ** -23 * np.abs(want)).all(), name
            np.testing.assert_array_equal(np.sign(g), np.sign(want), err_msg=name)   # the sign is exact
            np.testing.assert_array_equal(g[want == 0], 0.0)                        # and zero planes are exactly zero
        if name == "no_site":
            assert not g.any()                             # nothing valid outside class 0, classes 1 absent
    m, classes, ignore, _, _ = _pattern("bands6", shape_name)
    every = D.signed_distance(_dev(m), classes)            # class_ids=None: every class
    assert every.shape == (1, classes, h, w)
    np.testing.assert_array_equal(np.sign(every.cpu().numpy()), np.sign(R.signed_distance(m, classes)))


# ---- into the loss ---------------------------------------------------------------------------------------------------------
def test_weight_map_feeds_the_weighted_loss():
    """plumbing, not arithmetic: the map made on the device gives the loss, in bits, that the uploaded reference map gives"""
    from retinal_oct_image_segmentation_via_deep_learning_amd import losses
    D = _D()
    rng = np.random.default_rng(seed("loss"))
    t = R.wavy_bands(rng, (2, 16, 24), 4)
    t[:, :2, :] = 255
    t[:, :, 21:] = 255                                     # the border the augmenter fills
    wm = D.DistanceWeightMap.gaussian(4, 10.0, 2.0, ignore_index=255)
    want_w = R.weight_map(t, 4, wm.table.numpy(), 255)
    assert want_w.dtype == np.float32 and want_w.shape == (2, 16, 24) and len(np.unique(want_w)) > 4
    dt = _dev(t)
    logits = torch.from_numpy(rng.standard_normal((2, 4, 16, 24)).astype(np.float32)).cuda()
    res = []
    for w in (wm(dt), torch.from_numpy(want_w).cuda()):
        x = logits.clone().requires_grad_(True)
        loss = losses.cross_entropy_dice(x, dt, w_ce=1.0, w_dice=0.5, pixel_weight=w, ignore_index=255)
        loss.backward()
        res.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
    assert np.isfinite(res[0][0]) and np.abs(res[0][1]).max() > 0
    np.testing.assert_array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32))
    np.testing.assert_array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_raise_before_any_launch():
    D, L = _D(), _L()
    x = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    wm = D.DistanceWeightMap.boundary_bonus(3, 1.0)
    for call in (lambda t: D.squared_distance(t, 3, ["boundary"]), lambda t: D.signed_distance(t, 3), wm):
        with pytest.raises(L.OctError, match="no CPU fallback"):
            call(x.cpu())
        with pytest.raises(RuntimeError, match="16384"):
            call(torch.zeros(16385, 1, dtype=torch.uint8, device="cuda"))
    for bad in (0, 17):
        with pytest.raises(ValueError, match="classes"):
            D.squared_distance(x, bad, ["boundary"])
    with pytest.raises(ValueError, match="class of plane"):
        D.squared_distance(x, 3, [("class", 3)])
    with pytest.raises(ValueError, match="class of plane"):
        D.squared_distance(x, 3, ["boundary", ("other", 5)])
    with pytest.raises(ValueError, match="empty"):
        D.squared_distance(x, 3, [])
    with pytest.raises(ValueError, match="table is empty"):
        D.DistanceWeightMap(3, [])
    with pytest.raises(ValueError, match="class_ids"):
        D.signed_distance(x, 3, [3])
    # the library refuses the same on its own, before any launch: no pointer is looked at
    desc = L.DtDesc(2, 8, 8, 3, 0, 0, 1, 0, 0)
    assert L.lib().oct_dt_squared(C.byref(desc), (C.c_int32 * 2)(1, 3), None, None, None, None) == -22
    assert "names class" in L.last_error()
    assert L.lib().oct_dt_weight_map(C.byref(desc), (C.c_int32 * 2)(0, 0), None, None, 0, None, None, None) == -22
    assert "table is empty" in L.last_error()
