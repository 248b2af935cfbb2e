"""GPU: layer surfaces (csrc/surfaces.hip, surfaces.py, evaluation.SurfaceEvaluator) against the numpy restatement
tests/surf_ref.py, itself pinned to a brute force over all paths in test_surfaces_cpu.py.  Every comparison is == on whole
tensors; there are no tolerances.  Shapes: H in {1, 2, 63, 64, 65, 130} (one row, around the 64 rows of a cost tile, three tiles)
x W in {1, 2, 67} (around nothing, one column more than two cost tiles of 32), with K in {2, 9, 16} ordered classes (one, eight and
fifteen surfaces; K = 7 below takes the 8-wide kernels) and max_step in {None, 0, 1, 3, 32} (32 > H included); 257 x 300 crosses
the 256 threads of a search workgroup, the 256 columns of an arg-min strip and several tiles both ways."""
import functools
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import surf_ref as R
from oracle.bounds import seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HEIGHTS, WIDTHS, KS, STEPS = (1, 2, 63, 64, 65, 130), (1, 2, 67), (2, 9, 16), (None, 0, 1, 3, 32)


def _S():
    from retinal_oct_image_segmentation_via_deep_learning_amd import surfaces
    return surfaces


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


def _cuts(rng, b, h, w, k):
    """int [b, k-1, w]: ordered cuts that drift slowly along x"""
    base = np.sort(rng.integers(0, h + 1, size=(b, k - 1, 1)), axis=1)
    drift = np.cumsum(rng.integers(-1, 2, size=(b, k - 1, w)), axis=2)
    return np.maximum.accumulate(np.clip(base + drift, 0, h), axis=1)


@functools.lru_cache(maxsize=None)
def _inputs(h, w, k, b=1):
    """(classes, order, map int64 [b, h, w], scores fp32 [b, classes, h, w]), read-only: noisy bands of the k ordered classes
    (scrambled numbering) with a quarter of the labels replaced by anything in [0, classes], the last being out of range"""
    rng = np.random.default_rng(seed("surfaces", h, w, k))
    classes = min(16, k + 2)
    order = [int(c) for c in rng.permutation(classes)[:k]]
    pos = np.stack([R.band_map(h, w, c) for c in _cuts(rng, b, h, w, k)])
    clean = np.asarray(order)[pos]
    m = np.where(rng.random((b, h, w)) < 0.25, rng.integers(0, classes + 1, size=(b, h, w)), clean).astype(np.int64)
    z = rng.normal(size=(b, classes, h, w)).astype(np.float32)
    z += 1.5 * (np.arange(classes).reshape(1, -1, 1, 1) == clean[:, None]).astype(np.float32)
    m.setflags(write=False)
    z.setflags(write=False)
    return classes, order, m, z


def _bf16(z):
    """(the bf16 tensor, its values widened to fp32 as numpy)"""
    t = torch.from_numpy(np.array(z)).to(torch.bfloat16)
    return t, t.to(torch.float32).numpy()


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.unravel_index(bad.argmax(), bad.shape)}: " \
                          f"got {got[bad][0]} want {want[bad][0]}"


def _check_both_modes(h, w, k, step, b=1):
    """one map (uint8 or int64) and one score tensor (fp32 or bf16) through extract and paint"""
    classes, order, m, z = _inputs(h, w, k, b)
    pick = seed(h, w, k, step)
    ls = _S().LayerSurfaces(classes, order, max_step=step)
    # map mode
    mt = torch.from_numpy(m.copy())
    mt = (mt.to(torch.uint8) if pick & 1 else mt).cuda()
    want = R.extract(m, order, classes, step)
    got = ls.extract(mt)
    _same(got, want, f"map {mt.dtype} {h}x{w} K={k} step={step}")
    assert int(got.min()) >= 0 and int(got.max()) <= h
    _same(ls.paint(mt, got), R.paint(want, order, h).astype(m.dtype if mt.dtype == torch.int64 else np.uint8), "painted map")
    # scores mode
    if pick & 2:
        zt, zf = _bf16(z)
    else:
        zt, zf = torch.from_numpy(z.copy()), z
    want = R.extract_scores(zf, order, step)
    got = ls.extract_scores(zt.cuda())
    _same(got, want, f"scores {zt.dtype} {h}x{w} K={k} step={step}")
    _same(ls.paint(zt.cuda(), got), R.paint(want, order, h), "painted scores")


@pytest.mark.parametrize("step", STEPS, ids=lambda s: f"step{s}")
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_extract_and_paint_equal_the_restatement(h, w, k, step):
    _check_both_modes(h, w, k, step)


@pytest.mark.parametrize("step", (None, 3), ids=lambda s: f"step{s}")
def test_shape_across_workgroups_and_waves(step):
    _check_both_modes(257, 300, 9, step, b=2)


@pytest.mark.parametrize("step", (None, 1), ids=lambda s: f"step{s}")
def test_seven_classes_take_the_eight_wide_kernels(step):
    _check_both_modes(65, 67, 7, step, b=2)


@pytest.mark.parametrize("h", (600, 1100, 4095))
def test_tall_images_take_more_rows_per_search_thread(h):
    """four entries of s per thread of a 256-thread search workgroup, then 1024-thread workgroups with two and four; 4095 is the
    tallest image the entry points take"""
    _check_both_modes(h, 5, 2, 3)


# ---- dtypes and layouts -----------------------------------------------------------------------------------------------------------
def test_every_dtype_agrees_and_layouts_do_not_matter():
    classes, order, m, z = _inputs(65, 67, 9, b=5)
    for step in (None, 1):
        ls = _S().LayerSurfaces(classes, order, max_step=step)
        want = R.extract(m, order, classes, step)
        mt = torch.from_numpy(m.copy()).cuda()
        for dt in (torch.uint8, torch.int64, torch.int32, torch.int16):
            _same(ls.extract(mt.to(dt)), want, f"{dt} step={step}")
        # non-contiguous views: a transposed buffer, every second column of a wider one
        tr = mt.transpose(1, 2).contiguous().transpose(1, 2)
        assert not tr.is_contiguous()
        _same(ls.extract(tr), want, "transposed map")
        wide = torch.full((5, 65, 134), 3, dtype=torch.uint8, device="cuda")
        wide[:, :, ::2] = mt.to(torch.uint8)
        _same(ls.extract(wide[:, :, ::2]), want, "strided map")
        # extra leading dimensions: they come back in front of (K-1, W)
        lead = mt.reshape(1, 5, 1, 65, 67)
        got = ls.extract(lead)
        assert tuple(got.shape) == (1, 5, 1, 8, 67)
        _same(got.reshape(5, 8, 67), want, "leading dimensions")
        painted = ls.paint(lead, got)
        assert tuple(painted.shape) == tuple(lead.shape)
        _same(painted.reshape(5, 65, 67), R.paint(want, order, 65), "painted with leading dimensions")
        # scores: fp32, bf16, channels-last memory
        zt = torch.from_numpy(z.copy()).cuda()
        wz = R.extract_scores(z, order, step)
        _same(ls.extract_scores(zt), wz, "fp32 scores")
        _same(ls.extract_scores(zt.contiguous(memory_format=torch.channels_last)), wz, "channels-last scores")
        zb, zf = _bf16(z)
        _same(ls.extract_scores(zb.cuda()), R.extract_scores(zf, order, step), "bf16 scores")


# ---- free pixels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", (None, 0, 2), ids=lambda s: f"step{s}")
def test_free_pixels(step):
    rng = np.random.default_rng(seed("free", step))
    h, w, order, classes, ignore = 40, 45, [4, 1, 3, 0], 6, 3          # classes 2 and 5 are not ordered, 3 is ordered AND ignored
    pos = np.stack([R.band_map(h, w, c) for c in _cuts(rng, 4, h, w, 4)])
    m = np.asarray(order)[pos]
    m[0][rng.random((h, w)) < 0.3] = 2                                   # a class outside order
    m[1][rng.random((h, w)) < 0.3] = -7                                  # out of range (int64 only)
    m[1][rng.random((h, w)) < 0.2] = 250
    m[2, 10:25] = 5                                                      # whole free rows: flat stretches of N
    m[3] = 2                                                             # an all-free image
    ls = _S().LayerSurfaces(classes, order, max_step=step, ignore_index=ignore)
    want = R.extract(m, order, classes, step, ignore)
    _same(ls.extract(torch.from_numpy(m).cuda()), want, "int64 map with free pixels")
    assert (want[3] == 0).all()                                          # nothing to decide: the smallest s everywhere
    u8 = np.where(m < 0, 251, m).astype(np.uint8)
    _same(ls.extract(torch.from_numpy(u8).cuda()), R.extract(u8, order, classes, step, ignore), "uint8 map with free pixels")
    # ignore_index outside the classes altogether
    ls = _S().LayerSurfaces(classes, order, max_step=step, ignore_index=-7)
    _same(ls.extract(torch.from_numpy(m).cuda()), R.extract(m, order, classes, step, -7), "ignore_index -7")
    # scores: NaN frees a pixel whatever its channel, +-inf do not
    z = rng.normal(size=(3, classes, h, w)).astype(np.float32) + 2 * (np.arange(classes).reshape(1, -1, 1, 1) == m[:3, None])
    z = z.astype(np.float32)
    z[0][rng.random((classes, h, w)) < 0.05] = np.nan
    z[1][rng.random((classes, h, w)) < 0.05] = np.inf
    z[1][rng.random((classes, h, w)) < 0.05] = -np.inf
    z[2] = np.nan
    z[2, :, :5] = -np.inf                                                # every channel -inf: all equal the maximum
    ls = _S().LayerSurfaces(classes, order, max_step=step, keep=(2,))
    want = R.extract_scores(z, order, step)
    zt = torch.from_numpy(z).cuda()
    got = ls.extract_scores(zt)
    _same(got, want, "scores with NaN and infinities")
    cls = np.stack([R.argmax_first(zi) for zi in z])
    _same(ls.paint(zt, got), R.paint(want, order, h, keep=(2,), input_classes=cls), "painted scores with keep")


# ---- ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", (None, 0, 1, 32), ids=lambda s: f"step{s}")
def test_ties_take_the_smallest(step):
    h, w, order = 33, 70, [0, 1, 2]
    ls = _S().LayerSurfaces(3, order, max_step=step, scale=4.0, qmax=7)
    const = np.ones((1, h, w), dtype=np.int64)                          # one class: surface 1 at the top, surface 2 at the bottom
    want = R.extract(const, order, 3, step)
    assert (want[0, 0] == 0).all() and (want[0, 1] == h).all()
    _same(ls.extract(torch.from_numpy(const).cuda()), want, "constant map")
    zeros = np.zeros((2, 3, h, w), dtype=np.float32)                    # every N is 0 everywhere
    want = R.extract_scores(zeros, order, step, 4.0, 7)
    assert (want == 0).all()
    _same(ls.extract_scores(torch.from_numpy(zeros).cuda()), want, "all-zero scores")
    # rows of N that are equal: free rows and rows that cancel, in columns that disagree about where
    rng = np.random.default_rng(seed("ties"))
    m = np.zeros((2, h, w), dtype=np.int64)
    m[:, 12:] = 1
    m[:, 24:] = 2
    m[0, 8:16] = 7                                                       # free across the first boundary
    m[1, 10:14:2, :] = 1                                                 # 0 1 0 1 | 1 ...: N_1 returns to its minimum
    m[1, :, ::3] = np.roll(m[1, :, ::3], 2, axis=0)
    m[0][rng.random((h, w)) < 0.1] = 7
    ls7 = _S().LayerSurfaces(3, order, max_step=step)
    _same(ls7.extract(torch.from_numpy(m).cuda()), R.extract(m, order, 3, step), "equal rows of N")


def test_saturation_at_qmax():
    rng = np.random.default_rng(seed("saturation"))
    classes, order, m, _ = _inputs(65, 67, 9)
    z = (rng.normal(size=(1, classes, 65, 67)) * 40).astype(np.float32)  # margins far beyond qmax / scale
    for qmax, scale, step in ((1, 16.0, 1), (1, 0.001, None), (255, 16.0, 3), (3, 1e30, 1), (255, 1e-30, 0)):
        ls = _S().LayerSurfaces(classes, order, max_step=step, scale=scale, qmax=qmax)
        zt = torch.from_numpy(z).cuda()
        _same(ls.extract_scores(zt), R.extract_scores(z, order, step, np.float32(scale), qmax), f"qmax={qmax} scale={scale}")


# ---- chunks under the workspace limit ----------------------------------------------------------------------------------------------------
def test_three_chunks_equal_one():
    import ctypes as C
    S = _S()
    classes, order, m, z = _inputs(63, 67, 9, b=5)
    whole = S.LayerSurfaces(classes, order, max_step=3)
    one = int(S.L.lib().oct_surf_workspace_bytes(C.byref(whole._desc(1, 63, 67, torch.zeros(1, dtype=torch.int64), False))))
    assert one > 0
    split = S.LayerSurfaces(classes, order, max_step=3, max_workspace_bytes=2 * one + 17)      # 2 + 2 + 1 images
    mt, zt = torch.from_numpy(m.copy()).cuda(), torch.from_numpy(z.copy()).cuda()
    a, b = whole.extract(mt), split.extract(mt)
    assert split._workspace.numel() < whole._workspace.numel() and split._workspace.numel() <= 2 * one + 17
    assert torch.equal(a, b)
    _same(a, R.extract(m, order, classes, 3), "chunked maps")
    assert torch.equal(whole.extract_scores(zt), split.extract_scores(zt))
    with pytest.raises(RuntimeError, match="max_workspace_bytes"):
        S.LayerSurfaces(classes, order, max_step=3, max_workspace_bytes=one - 1).extract(mt)
    # without a step limit there is no workspace and no limit to respect
    free = S.LayerSurfaces(classes, order, max_step=None, max_workspace_bytes=1)
    _same(free.extract(mt), R.extract(m, order, classes, None), "no workspace")
    assert free._workspace is None


# ---- paint ------------------------------------------------------------------------------------------------------------------------------
def test_paint_keep_and_in_place():
    rng = np.random.default_rng(seed("paint"))
    h, w, order, classes = 70, 300, [1, 2, 0, 5], 7
    pos = np.stack([R.band_map(h, w, c) for c in _cuts(rng, 3, h, w, 4)])
    m = np.asarray(order)[pos]
    m[rng.random(m.shape) < 0.2] = 3                                     # fluid: kept
    m[rng.random(m.shape) < 0.1] = 4                                     # another class outside order: painted over
    m[rng.random(m.shape) < 0.05] = 9                                    # out of range: painted over
    ls = _S().LayerSurfaces(classes, order, max_step=2, keep=(3, 6))
    for dt in (np.int64, np.uint8):
        mt = torch.from_numpy(m.astype(dt)).cuda()
        s = ls.extract(mt)
        want_s = R.extract(m, order, classes, 2)
        _same(s, want_s, "surfaces")
        want = R.paint(want_s, order, h, keep=(3, 6), input_classes=m).astype(dt)
        assert (want == 3).any() and not (want == 4).any() and not (want == 9).any()
        _same(ls.paint(mt, s), want, f"painted {dt.__name__}")
        _same(ls(mt), want, "__call__")
        # arbitrary surfaces, not ordered: the count rule
        anys = rng.integers(0, h + 1, size=(3, 3, w)).astype(np.int32)
        _same(ls.paint(mt, torch.from_numpy(anys).cuda()), R.paint(anys, order, h, keep=(3, 6), input_classes=m).astype(dt), "any surfaces")
        out = torch.empty_like(mt)
        assert ls.paint(mt, s, out=out) is out
        _same(out, want, "out=")
        assert ls.paint(mt, s, out=mt) is mt                             # in place
        _same(mt, want, "in place")
        with pytest.raises(RuntimeError, match="out must be"):
            ls.paint(mt, s, out=torch.empty(3, h, w, dtype=torch.int32, device="cuda"))
    # scores: the kept class comes from the arg-max
    z = rng.normal(size=(3, classes, h, w)).astype(np.float32) + 2 * (np.arange(classes).reshape(1, -1, 1, 1) == m[:, None])
    z = z.astype(np.float32)
    zt = torch.from_numpy(z).cuda()
    s = ls.extract_scores(zt)
    want_s = R.extract_scores(z, order, 2)
    _same(s, want_s, "score surfaces")
    want = R.paint(want_s, order, h, keep=(3, 6), input_classes=z.argmax(axis=1))
    assert (want == 3).any()
    out = torch.empty((3, h, w), dtype=torch.int64, device="cuda")
    assert ls.paint(zt, s, out=out) is out
    _same(out, want, "painted scores")
    zb, zf = _bf16(z)
    _same(ls.paint(zb.cuda(), s), R.paint(want_s, order, h, keep=(3, 6), input_classes=zf.argmax(axis=1)), "painted bf16 scores")


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------
def test_surface_evaluator_state_equals_numpy_sums():
    E = _E()
    rng = np.random.default_rng(seed("evaluator"))
    t = rng.integers(0, 4096, size=(30, 7, 301)).astype(np.int32)      # 9030 columns: more than the 32 x 256 threads of a surface
    p = rng.integers(0, 4096, size=(30, 7, 301)).astype(np.int32)
    valid = rng.random((30, 301)) < 0.7
    valid[2] = False
    tt, pt, vt = torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(valid).cuda()
    ev = E.SurfaceEvaluator(7)
    ev.update(tt, pt)
    _same(ev.state.view(7, 5), R.error_state(t, p), "one update")
    m = ev.compute()
    want = E.surface_metrics_from_state(R.error_state(t, p), 7)
    for key in want:
        np.testing.assert_array_equal(m[key], want[key], err_msg=key)
    assert m["columns"].tolist() == [30 * 301] * 7 and 0 < m["mean_mean_abs_error"] < 4096
    # two updates equal one update on the concatenation
    two = E.SurfaceEvaluator(7, device="cuda")
    two.update(tt[:2], pt[:2]).update(tt[2:], pt[2:])
    assert torch.equal(two.state, ev.state)
    # the valid mask, bool and uint8, and leading dimensions
    ev.reset()
    assert int(ev.state.abs().sum()) == 0
    ev.update(tt, pt, vt)
    _same(ev.state.view(7, 5), R.error_state(t, p, valid), "valid mask")
    other = E.SurfaceEvaluator(7)
    other.update(tt.reshape(2, 15, 7, 301), pt.reshape(2, 15, 7, 301), vt.reshape(2, 15, 301).to(torch.uint8))
    assert torch.equal(other.state, ev.state)
    none = E.SurfaceEvaluator(7).update(tt, pt, torch.zeros(30, 301, dtype=torch.bool, device="cuda"))
    assert int(none.state.abs().sum()) == 0 and np.isnan(none.compute()["mean_rmse"])
    # one column, one surface
    tiny = E.SurfaceEvaluator(1).update(torch.tensor([[[5]]], dtype=torch.int32).cuda(), torch.tensor([[[2]]], dtype=torch.int32).cuda())
    assert tiny.state.tolist() == [1, 3, -3, 9, 3]
    assert tiny.compute()["mean_signed_error"].tolist() == [-3.0]


def test_surface_evaluator_update_maps():
    S, E = _S(), _E()
    rng = np.random.default_rng(seed("update_maps"))
    h, w, k, ignore = 48, 64, 5, 255
    cuts = _cuts(rng, 4, h, w, k)
    target = np.stack([R.band_map(h, w, c) for c in cuts])
    pred = np.where(rng.random(target.shape) < 0.3, rng.integers(0, k, size=target.shape), target)
    target[:, :, 10:20] = ignore                                         # whole columns without a label: not counted
    target[1, 5:9, 30:40] = ignore                                       # a few ignored pixels: the column still counts
    valid = (target != ignore).any(axis=-2)
    assert not valid[:, 10:20].any() and valid[:, 30:40].all()
    ls = S.LayerSurfaces(k, range(k), max_step=1, ignore_index=ignore)
    ts = R.extract(target, range(k), k, None, ignore)
    ps = R.extract(pred, range(k), k, 1, ignore)
    for dt in (torch.int64, torch.uint8):
        ev = E.SurfaceEvaluator(k - 1)
        ev.update_maps(torch.from_numpy(target).to(dt).cuda(), torch.from_numpy(pred).to(dt).cuda(), ls)
        _same(ev.state.view(k - 1, 5), R.error_state(ts, ps, valid), f"update_maps {dt}")
    # outside the ignored columns the target's unconstrained surfaces are its boundaries
    assert (ts[:, :, 20:30] == cuts[:, :, 20:30]).all()
    # without ignore_index every column counts
    clean = np.stack([R.band_map(h, w, c) for c in cuts])
    ev = E.SurfaceEvaluator(k - 1)
    plain = S.LayerSurfaces(k, range(k), max_step=None)
    ev.update_maps(torch.from_numpy(clean).cuda(), torch.from_numpy(pred).cuda(), plain)
    _same(ev.state.view(k - 1, 5), R.error_state(cuts.astype(np.int32), R.extract(pred, range(k), k, None)), "no ignore_index")
    assert ev.compute()["columns"].tolist() == [4 * w] * (k - 1)


# ---- two ranks: the sums add, the largest |e| is a maximum ----------------------------------------------------------------------------
def _rank_surfaces():
    rng = np.random.default_rng(33)
    t = rng.integers(0, 200, size=(5, 3, 70)).astype(np.int32)      # 5 images: shards of 3 and 2
    p = t + rng.integers(-9, 10, size=t.shape).astype(np.int32)
    p[4, 1, 7] = t[4, 1, 7] + 150                                    # the largest |e| of surface 1 lies in rank 1's shard,
    p[0, 2, 3] = t[0, 2, 3] - 120                                    # that of surface 2 in rank 0's
    return t, p


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    import datetime
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp, evaluation
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    t, p = _rank_surfaces()
    lo, hi = ddp.shard_batch(t.shape[0], rank, world)
    ev = evaluation.SurfaceEvaluator(3)
    ev.update(torch.from_numpy(t[lo:hi]).cuda(), torch.from_numpy(p[lo:hi]).cuda())
    local = ev.state.cpu().numpy().copy()
    ev.all_reduce()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), state=ev.state.cpu().numpy(), local=local, lo=lo, hi=hi)
    dist.destroy_process_group()


def test_two_ranks_all_reduce_sums_the_sums_and_takes_the_largest_error(tmp_path):
    world = 2
    ctx = mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=False)
    deadline = time.monotonic() + 180                                # a guard for every child, not a wait: join returns at exit
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("a rank did not finish within 180 s")
    t, p = _rank_surfaces()
    want = R.error_state(t, p).reshape(-1)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["lo"]) == 0 and int(r0["hi"]) == int(r1["lo"]) and int(r1["hi"]) == 5
    np.testing.assert_array_equal(r0["state"], r1["state"])
    np.testing.assert_array_equal(r0["state"], want)
    l0, l1 = r0["local"].reshape(3, 5), r1["local"].reshape(3, 5)
    np.testing.assert_array_equal(l0, R.error_state(t[:3], p[:3]))
    np.testing.assert_array_equal((l0 + l1)[:, :4], want.reshape(3, 5)[:, :4])
    assert l0[1, 4] < l1[1, 4] == 150 and l1[2, 4] < l0[2, 4] == 120      # a sum of the two would be wrong in both
    np.testing.assert_array_equal(np.maximum(l0, l1)[:, 4], want.reshape(3, 5)[:, 4])
    # one process, no group: nothing to do
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    ev = evaluation.SurfaceEvaluator(3).update(torch.from_numpy(t).cuda(), torch.from_numpy(p).cuda())
    assert ev.all_reduce() is ev
    _same(ev.state, want, "single process")


# ---- from a model -----------------------------------------------------------------------------------------------------------------------
def test_from_model_equals_extract_scores_of_its_logits():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    torch.manual_seed(5)
    model = UNet(1, 2, init_features=4).cuda().eval()
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(6)).cuda()
    ls = _S().LayerSurfaces(2, [0, 1], max_step=1)
    logits = model.logits(x)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (2, 2, 32, 48)
    got = ls.from_model(model, x)
    assert torch.equal(got, ls.extract_scores(logits))
    _same(got, R.extract_scores(logits.cpu().numpy(), [0, 1], 1), "from_model")
    painted = ls.paint(logits, got)
    _same(painted, R.paint(got.cpu().numpy(), [0, 1], 32), "painted")
    assert (painted[:, 1:] >= painted[:, :-1]).all()                     # ordered top to bottom: no holes, no islands
