"""GPU: connected components (csrc/components.hip, postprocess, evaluation.LesionEvaluator) against the numpy restatement
tests/cc_ref.py.  Everything is integers: every comparison is == on whole tensors.  The shapes come from oct_cc_tile, so they keep
straddling tile borders if the tile changes: one pixel, one row and one column over three tiles, exactly one tile, one tile plus
one pixel each way (four tiles, three of them slivers), three tiles each way with ragged edges.  The patterns are the ones that
break a labelling: noise of 2, 3 and 9 classes, 2-class noise near the 4-connectivity percolation threshold (large tortuous
components through every tile), a serpentine and a spiral (one component crossing every tile border many times), the two
diagonals through a tile corner, one class everywhere, every pixel ignored, labels out of range."""
import functools

import numpy as np
import pytest
import torch

import cc_ref as R
from oracle.bounds import seed

pytestmark = pytest.mark.gpu

IGNORE = 5
SHAPE_NAMES = ("pixel", "row", "column", "tile", "tile_plus_one", "three_tiles")
PATTERNS = ("noise2", "noise2_p59", "noise3", "noise9", "serpentine", "spiral", "diagonal", "antidiagonal", "one_class",
            "all_ignored", "out_of_range_u8", "out_of_range_i64")


def _P():
    from retinal_oct_image_segmentation_via_deep_learning_amd import postprocess
    return postprocess


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


@functools.lru_cache(maxsize=None)
def _shape(name):
    th, tw = _P().tile()
    return {"pixel": (1, 1), "row": (1, 2 * tw + 3), "column": (2 * th + 3, 1), "tile": (th, tw), "tile_plus_one": (th + 1, tw + 1),
            "three_tiles": (2 * th + 3, 2 * tw + 5)}[name]


@functools.lru_cache(maxsize=None)
def _pattern(name, shape_name, images=1):
    """(int64 map [images, h, w], classes, ignore_index, fits uint8) -- None where the shape cannot hold the pattern"""
    h, w = _shape(shape_name)
    th, tw = _P().tile()
    rng = np.random.default_rng(seed(name, shape_name, images))
    classes, ignore, u8 = 2, None, True
    if name in ("noise2", "noise3", "noise9"):
        classes = int(name[5:])
        m = rng.integers(0, classes, size=(images, h, w))
    elif name == "noise2_p59":
        m = (rng.random((images, h, w)) < 0.59).astype(np.int64)
    elif name == "serpentine":
        m = np.stack([R.serpentine(h, w)] * images)
    elif name == "spiral":
        m = np.stack([R.spiral(h, w)] * images)
    elif name in ("diagonal", "antidiagonal"):
        if h <= th or w <= tw:
            return None
        m = np.zeros((images, h, w), dtype=np.int64)
        if name == "diagonal":
            m[:, th - 1, tw - 1] = m[:, th, tw] = 1
        else:
            m[:, th - 1, tw] = m[:, th, tw - 1] = 1
    elif name == "one_class":
        classes = 3
        m = np.full((images, h, w), 2, dtype=np.int64)
    elif name == "all_ignored":
        classes, ignore = 9, IGNORE
        m = np.full((images, h, w), IGNORE, dtype=np.int64)
    elif name == "out_of_range_u8":
        classes, ignore = 3, 1
        m = rng.integers(0, 3, size=(images, h, w))
        m[rng.random(m.shape) < 0.2] = 200
    else:
        classes, u8 = 3, False
        m = rng.integers(0, 3, size=(images, h, w))
        r = rng.random(m.shape)
        m[r < 0.15] = -5
        m[r > 0.85] = 2 ** 40
    m = m.astype(np.int64)
    m.setflags(write=False)
    return m, classes, ignore, u8


@functools.lru_cache(maxsize=None)
def _ref(name, shape_name, connectivity, images=1):
    m, classes, ignore, _ = _pattern(name, shape_name, images)
    roots, info = R.label(m, classes, connectivity, ignore)
    roots.setflags(write=False)
    info.setflags(write=False)
    return roots, info


def _dev(a, dtype=torch.int64):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()   # a copy: the cached cases are read-only


def _offset_by_one(t):
    """the same values in a buffer whose base is one element past an aligned allocation"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_roots_and_info_match_the_restatement(shape_name, connectivity):
    P = _P()
    for name in PATTERNS:
        case = _pattern(name, shape_name)
        if case is None:
            continue
        m, classes, ignore, u8 = case
        want_roots, want_info = _ref(name, shape_name, connectivity)
        got = []
        for dtype in ((torch.uint8, torch.int64) if u8 else (torch.int64,)):
            for shift in (False, True):
                x = _dev(m, dtype)
                x = _offset_by_one(x) if shift else x
                roots, info = P.connected_components(x, classes, connectivity, ignore)
                again = P.connected_components(x, classes, connectivity, ignore)
                assert roots.dtype == torch.int32 and info.dtype == torch.int32 and roots.shape == x.shape
                assert torch.equal(roots, again[0]) and torch.equal(info, again[1]), f"{name}: two runs differ"
                got.append((roots.cpu().numpy(), info.cpu().numpy()))
        print(shape_name, connectivity, name, "components", int((want_info != 0).sum()), "largest",
              int((want_info & ((1 << R.BORDER_BIT) - 1)).max()))
        for roots, info in got:                          # uint8 and int64, aligned and offset: all the same bits
            np.testing.assert_array_equal(roots, want_roots, err_msg=f"roots {name}")
            np.testing.assert_array_equal(info, want_info, err_msg=f"info {name}")
        if name == "one_class":
            h, w = m.shape[-2:]
            edge = 1 << R.BORDER_BIT
            assert got[0][1][0, 0, 0] == (h * w | edge) and (got[0][0] == 0).all()
        if name == "all_ignored":
            assert (got[0][0] == -1).all() and not got[0][1].any()
        if name in ("diagonal", "antidiagonal"):         # one component at 8-connectivity, two at 4
            cls1 = got[0][0][m == 1]
            assert len(np.unique(cls1)) == (1 if connectivity == 8 else 2)
        if name in ("serpentine", "spiral"):
            assert len(np.unique(got[0][0][m == 1])) == 1


@pytest.mark.parametrize("lead", [(3,), (2, 2)], ids=["3", "2x2"])
def test_several_images_and_leading_dimensions(lead):
    P = _P()
    images = int(np.prod(lead))
    for name in ("noise3", "noise2_p59", "out_of_range_i64"):
        m, classes, ignore, u8 = _pattern(name, "three_tiles", images)
        for connectivity in (4, 8):
            want_roots, want_info = _ref(name, "three_tiles", connectivity, images)
            x = _dev(m, torch.uint8 if u8 else torch.int64).reshape(lead + m.shape[-2:])
            roots, info = P.connected_components(x, classes, connectivity, ignore)
            assert roots.shape == x.shape
            np.testing.assert_array_equal(roots.cpu().numpy().reshape(want_roots.shape), want_roots)
            np.testing.assert_array_equal(info.cpu().numpy().reshape(want_info.shape), want_info)


def test_component_table_matches_the_restatement():
    P = _P()
    for name, shape_name, images in (("noise3", "three_tiles", 3), ("noise9", "tile_plus_one", 1), ("all_ignored", "tile", 1),
                                     ("out_of_range_u8", "three_tiles", 1)):
        m, classes, ignore, _ = _pattern(name, shape_name, images)
        for connectivity in (4, 8):
            got = P.component_table(_dev(m, torch.uint8), classes, connectivity, ignore)
            assert got.dtype == torch.int64 and got.is_cuda
            assert torch.equal(got, P.component_table(_dev(m, torch.int64), classes, connectivity, ignore)), "two runs differ"
            np.testing.assert_array_equal(got.cpu().numpy(), R.table(m, classes, connectivity, ignore))


RULES = {
    "min_area": dict(min_area=[0, 3, 5]),
    "keep_largest": dict(keep_largest=[0, 1, 1]),
    "fill_enclosed": dict(fill_enclosed=[1, 0, 1], replace=[1, 0, 0]),
    "all": dict(min_area=[2, 0, 4], keep_largest=[0, 1, 0], fill_enclosed=[1, 1, 0], replace=[2, 0, 1]),
    "scalar": dict(min_area=4, replace=7),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_filter_rules_match_the_restatement(rule):
    P = _P()
    kw = RULES[rule]
    for name, shape_name, images in (("noise3", "three_tiles", 2), ("noise3", "tile_plus_one", 1), ("out_of_range_u8", "three_tiles", 1),
                                     ("out_of_range_i64", "three_tiles", 1), ("noise3", "pixel", 1)):
        m, classes, ignore, u8 = _pattern(name, shape_name, images)
        for connectivity in (4, 8):
            want = R.filter_map(m, classes, connectivity=connectivity, ignore_index=ignore, **kw)
            flt = P.ComponentFilter(classes, connectivity=connectivity, ignore_index=ignore, **kw)
            for dtype in ((torch.uint8, torch.int64) if u8 else (torch.int64,)):
                x = _dev(m, dtype)
                keep = x.clone()
                out = flt(x)
                assert out.dtype == dtype and out.shape == x.shape and torch.equal(x, keep)
                np.testing.assert_array_equal(out.cpu().numpy().astype(np.int64), want, err_msg=f"{name} {dtype}")
                assert torch.equal(flt(x), out), "two runs differ"
                same = flt(x, out=x)                     # in place
                assert same is x and torch.equal(x, out)
                y = _offset_by_one(keep)
                assert torch.equal(flt(y), out)


def test_filter_masks_treats_every_channel_as_a_two_class_image():
    P = _P()
    h, w = _shape("three_tiles")
    rng = np.random.default_rng(seed("masks"))
    mask = (rng.random((2, 3, h, w)) < 0.6).astype(np.uint8)
    for kw in (dict(fill_enclosed=[1, 0], replace=[1, 0]), dict(min_area=[0, 6], keep_largest=[0, 1])):
        for connectivity in (4, 8):
            flt = P.ComponentFilter(2, connectivity=connectivity, **kw)
            got = flt.filter_masks(_dev(mask, torch.uint8))
            assert got.dtype == torch.uint8 and got.shape == (2, 3, h, w)
            assert torch.equal(got, flt.filter_masks(_dev(mask, torch.uint8))), "two runs differ"
            np.testing.assert_array_equal(got.cpu().numpy(), R.filter_map(mask, 2, connectivity=connectivity, **kw))


# ---- lesion-wise counts -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(shape_name, images, classes, ignore):
    """(target, pred): blobs on a background, the prediction a shifted and perturbed copy; some pixels ignored / out of range"""
    h, w = _shape(shape_name)
    rng = np.random.default_rng(seed("pair", shape_name, images, classes, ignore))
    coarse = rng.integers(0, classes, size=(images, (h + 3) // 4, (w + 3) // 4))
    coarse[rng.random(coarse.shape) < 0.5] = 0
    t = np.repeat(np.repeat(coarse, 4, axis=1), 4, axis=2)[:, :h, :w].astype(np.int64)
    p = np.roll(t, (1, 2), axis=(1, 2))
    flip = rng.random(p.shape) < 0.05
    p[flip] = rng.integers(0, classes, size=int(flip.sum()))
    p[rng.random(p.shape) < 0.01] = classes + 3          # invalid
    if ignore is not None:
        t[rng.random(t.shape) < 0.1] = ignore
    t.setflags(write=False)
    p.setflags(write=False)
    return t, p


def _state(ev):
    return ev.state.cpu().numpy()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("ignore", [None, 255])
def test_lesion_state_matches_the_restatement(ignore, connectivity):
    E = _E()
    for shape_name, images, classes, overlap in (("three_tiles", 2, 3, (0, 1)), ("three_tiles", 1, 9, (1, 2)), ("tile_plus_one", 3, 2, (1, 1)),
                                                 ("pixel", 1, 2, (0, 1)), ("row", 2, 3, (1, 3))):
        t, p = _pair(shape_name, images, classes, ignore)
        want = R.lesion_state(t, p, classes, connectivity, ignore, overlap)
        for td, pd in ((torch.uint8, torch.int64), (torch.int64, torch.uint8)):
            ev = E.LesionEvaluator(classes, connectivity, ignore, overlap).update(_dev(t, td), _dev(p, pd))
            print(shape_name, classes, overlap, _state(ev))
            np.testing.assert_array_equal(_state(ev), want, err_msg=f"{shape_name} {classes} {overlap}")
            again = E.LesionEvaluator(classes, connectivity, ignore, overlap).update(_dev(t, td), _dev(p, pd))
            assert torch.equal(ev.state, again.state)
        m = ev.compute()
        np.testing.assert_array_equal(m["detected"], want[:classes * 4].reshape(classes, 4)[:, 2])
        assert m["images"] == images and m["updates"] == 1


def test_lesion_updates_add_up_and_chunks_change_nothing():
    E = _E()
    t, p = _pair("three_tiles", 3, 3, 255)
    whole = R.lesion_state(t, p, 3, 4, 255, (1, 4))
    parts = R.lesion_state(t[:1], p[:1], 3, 4, 255, (1, 4)) + R.lesion_state(t[1:], p[1:], 3, 4, 255, (1, 4))
    np.testing.assert_array_equal(parts[:-1], whole[:-1])  # a component never spans two images; only `updates` differs
    td, pd = _dev(t, torch.uint8), _dev(p, torch.uint8)
    ev = E.LesionEvaluator(3, 4, 255, (1, 4)).update(td[:1], pd[:1]).update(td[1:], pd[1:])
    np.testing.assert_array_equal(_state(ev), parts)
    h, w = t.shape[-2:]
    one = E.LesionEvaluator(3, 4, 255, (1, 4), max_workspace_bytes=27 * h * w + 8 * 256)   # room for one image, not for two
    one.update(td.reshape(3, 1, h, w), pd.reshape(3, 1, h, w))
    got = _state(one)
    np.testing.assert_array_equal(got[:-1], whole[:-1])
    assert got[-1] == 3                                   # three chunks of one image
    with pytest.raises(RuntimeError, match="max_workspace_bytes"):
        E.LesionEvaluator(3, max_workspace_bytes=h * w).update(td, pd)
    assert not _state(ev.reset()).any()


def test_lesion_known_answers_ignore_rule_and_overlap_at_equality():
    E = _E()
    t = np.zeros((1, 4, 8), dtype=np.int64)
    p = np.zeros((1, 4, 8), dtype=np.int64)
    t[0, 1, 1:5] = 1
    p[0, 1, 4:6] = 1
    for overlap, want in (((1, 4), [1, 1, 1, 1]), ((1, 2), [1, 1, 0, 1]), ((3, 4), [1, 1, 0, 0])):
        ev = E.LesionEvaluator(2, min_overlap=overlap).update(_dev(t), _dev(p))
        np.testing.assert_array_equal(_state(ev)[4:8], want)
    t = np.zeros((3, 7), dtype=np.int64)
    p = np.zeros((3, 7), dtype=np.int64)
    p[1, 1:6] = 1
    t[1, 3] = 255
    t[1, 5] = 1
    p[0, 0] = 9
    ev = E.LesionEvaluator(2, ignore_index=255).update(_dev(t), _dev(p))
    np.testing.assert_array_equal(_state(ev)[4:], [1, 2, 1, 1, 1, 1, 1, 1])   # the ignored pixel splits the prediction
    ev = E.LesionEvaluator(2).update(_dev(t, torch.uint8), _dev(p, torch.uint8))
    np.testing.assert_array_equal(_state(ev), R.lesion_state(t, p, 2))


def test_update_model_equals_update_on_the_prediction():
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    E = _E()
    torch.manual_seed(3)
    model = M.MGUNet_2(1, 3, feature_scale=16).cuda().eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 48, 64, generator=g).cuda()
    target = torch.randint(0, 3, (2, 12, 16), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2).cuda()
    pred = model.predict(x)
    a = E.LesionEvaluator(3, 8).update_model(model, x, target)
    b = E.LesionEvaluator(3, 8).update(target, pred)
    assert torch.equal(a.state, b.state)
    np.testing.assert_array_equal(_state(a), R.lesion_state(target.cpu().numpy(), pred.cpu().numpy(), 3, 8))
    with pytest.raises(RuntimeError, match="classes"):
        E.LesionEvaluator(4).update_model(model, x, target)
