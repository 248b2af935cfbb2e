"""GPU: the streaming evaluator (csrc/seg_eval.hip, evaluation.SegEvaluator) against the int64 restatement tests/eval_ref.py.
Every comparison is on integers and exact; the float formulas are compared with == against the same formulas on the
restatement's counts.  Shapes are the smallest at which the kernel can go wrong: one pixel, odd tails, more than one strip of
64 (int64) / 128 (uint8 pair) columns, more rows than one round of the waves, leading dimensions, a misaligned view."""
import functools
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import eval_ref as R
from oracle.bounds import Out, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 5, 7), (3, 33, 130), (2, 19, 300), (1, 70, 64), (2, 3, 4, 40)]
CLASSES = [1, 2, 3, 8, 9, 11, 16]
KINDS = ("layered", "random", "one_class")
DTYPES = {"u8": torch.uint8, "i64": torch.int64}
IGNORE = {"u8": 255, "i64": -100}


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


@functools.lru_cache(maxsize=None)
def _maps(shape, classes, kind, ignore):
    """(target, pred, reference state): computed once per case, never modified"""
    rng = np.random.default_rng(seed(shape, classes, kind, ignore))
    if kind == "layered":
        t, p = R.layered_maps(rng, shape, classes)
    elif kind == "random":
        t, p = R.random_maps(rng, shape, classes)
    else:   # every pixel in one bin: the maximum-conflict case
        t = np.full(shape, classes - 1, dtype=np.int64)
        p = t.copy()
    if ignore is not None:
        t = t.copy()
        t[rng.random(shape) < 0.25] = ignore
    t.setflags(write=False)
    p.setflags(write=False)
    ref = R.eval_state(t, p, classes, ignore)
    ref.setflags(write=False)
    return t, p, ref


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _state(ev):
    return ev.state.cpu().numpy()


@pytest.mark.parametrize("classes", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_class_maps_match_the_restatement(shape, classes):
    E = _E()
    for kind in KINDS:
        for tn, tdt in DTYPES.items():
            for ignore in (None, IGNORE[tn]):
                t, p, ref = _maps(shape, classes, kind, ignore)
                for pn, pdt in DTYPES.items():
                    ev = E.SegEvaluator(classes, ignore_index=ignore)
                    ev.update(_dev(t, tdt), _dev(p, pdt))
                    got = _state(ev)
                    print(shape, classes, kind, tn, pn, ignore, "cm sum", got[:classes * classes].sum(), "ignored", got[-3])
                    np.testing.assert_array_equal(got, ref, err_msg=f"{kind} target {tn} pred {pn} ignore {ignore}")
                    if kind == "one_class" and ignore is None:
                        assert got[classes * classes - 1] == t.size          # cm[c][c] == n
    m = ev.compute()
    assert m["updates"] == 1 and m["columns"] == int(np.prod(shape[:-2])) * shape[-1]


@pytest.mark.parametrize("which", ["target", "pred", "both"])
def test_misaligned_uint8_views(which):
    """maps[1:] of a 5 x 7 uint8 batch starts 35 bytes into its storage"""
    E = _E()
    t, p, _ = _maps((4, 5, 7), 3, "random", None)
    dt, dp = _dev(t, torch.uint8), _dev(p, torch.uint8)
    vt = dt[1:] if which in ("target", "both") else dt[1:].clone()
    vp = dp[1:] if which in ("pred", "both") else dp[1:].clone()
    assert (vt.data_ptr() % 16 != 0 or which == "pred") and (vp.data_ptr() % 16 != 0 or which == "target")
    ev = E.SegEvaluator(3).update(vt, vp)
    np.testing.assert_array_equal(_state(ev), R.eval_state(t[1:], p[1:], 3))


@pytest.mark.parametrize("classes", [1, 3, 16])
@pytest.mark.parametrize("tn,pn", [("u8", "u8"), ("u8", "i64"), ("i64", "u8"), ("i64", "i64")])
def test_out_of_range_labels_land_in_invalid_and_nothing_is_written_outside(tn, pn, classes):
    E = _E()
    shape = (2, 19, 150)
    rng = np.random.default_rng(seed(tn, pn, classes))
    t, p = (a.copy() for a in R.layered_maps(rng, shape, classes))
    clean = R.eval_state(t, p, classes)
    bad = {"u8": [classes, 200, 255], "i64": [classes, -1, -2 ** 63, 2 ** 63 - 1, 2 ** 40, 256 + classes - 1]}
    mt, mp_ = rng.random(shape) < 0.07, rng.random(shape) < 0.07
    t[mt] = rng.choice(bad[tn], size=int(mt.sum()))
    p[mp_] = rng.choice(bad[pn], size=int(mp_.sum()))
    ref = R.eval_state(t, p, classes)
    assert ref[-2] == int((mt | mp_).sum()) > 0
    out = Out((E.state_size(classes),), torch.int64, fill=-7777)
    out.t.zero_()
    ev = E.SegEvaluator(classes)
    ev.state = out.t
    ev.update(_dev(t, DTYPES[tn]), _dev(p, DTYPES[pn]))
    got = out.host()                                             # asserts the sentinel tail
    np.testing.assert_array_equal(got, ref)
    # everything else is unaffected: the valid pixels count exactly as if the others were not there
    keep = ~(mt | mp_)
    assert got[:classes * classes].sum() == int(keep.sum()) and got[-3] == 0
    assert (got[:classes * classes] <= clean[:classes * classes]).all()


def test_three_updates_accumulate_without_a_synchronisation_and_reset_zeroes():
    E = _E()
    cases = [_maps((3, 33, 130), 8, "layered", -100), _maps((2, 19, 300), 8, "random", -100), _maps((1, 70, 64), 8, "layered", -100)]
    dev = [(_dev(t, torch.int64), _dev(p, torch.int64)) for t, p, _ in cases]
    ev = E.SegEvaluator(8, ignore_index=-100)
    ev.update(*dev[0]).reset()                                   # state allocated, then zero
    assert not _state(ev).any()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t, p in dev:
            ev.update(t, p)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    np.testing.assert_array_equal(_state(ev), sum(ref for _, _, ref in cases))
    m = ev.compute()
    assert m["updates"] == 3 and m["columns"] == 3 * 130 + 2 * 300 + 64
    ev.reset()
    assert not _state(ev).any() and ev.compute()["updates"] == 0


def test_updates_on_a_side_stream_are_ordered_on_that_stream():
    """update and update_logits inside torch.cuda.stream(s): the state is allocated and both kernels run on s, the stream of
    the tensors' device, so s.synchronize() alone makes the state readable.  Width 70: one full strip of 64 columns and a tail."""
    E = _E()
    t, p, ref = _maps((2, 5, 70), 3, "random", 255)
    lg = np.random.default_rng(seed("side stream")).standard_normal((2, 5, 70, 3)).astype(np.float32)
    dt, dp, dl = _dev(t, torch.uint8), _dev(p, torch.uint8), torch.from_numpy(lg).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                   # the inputs were written on the default stream
    ev = E.SegEvaluator(3, ignore_index=255)
    with torch.cuda.stream(s):
        ev.update(dt, dp).update_logits(dt, dl, "nhwc")
    s.synchronize()
    np.testing.assert_array_equal(_state(ev), ref + R.eval_state(t, R.argmax_first(lg, 3), 3, 255))
    assert ev.compute()["updates"] == 2


@pytest.mark.parametrize("classes", [2, 8, 11])
def test_counts_equal_metrics_evaluate_and_thickness_equals_the_reference_function(classes):
    from retinal_oct_image_segmentation_via_deep_learning_amd import Metrics
    E = _E()
    t, p, ref = _maps((3, 33, 130), classes, "layered", None)
    dt, dp = _dev(t, torch.int64), _dev(p, torch.int64)
    m = E.SegEvaluator(classes).update(dt, dp).compute()
    old = Metrics.evaluate(dt, dp, classes=classes)
    np.testing.assert_array_equal(m["counts"], old["counts"])
    for k in old:
        if k != "counts":
            assert (m[k] == old[k]).all(), k
    np.testing.assert_array_equal(Metrics.confusion_matrix(t, p, classes), ref[:classes * classes].reshape(classes, classes))
    np.testing.assert_array_equal(Metrics.confusion_matrix(dt, dp, classes), m["confusion"])
    # one 2-D image: thickness_error[c] * W against the reference's thickness_difference(t == c, p == c) * W
    t2, p2 = t[1], p[1]
    w = t2.shape[1]
    m2 = E.SegEvaluator(classes).update(_dev(t2, torch.uint8), _dev(p2, torch.uint8)).compute()
    for c in range(classes):
        assert m2["thickness_error"][c] * w == R.thickness_difference(t2 == c, p2 == c) * w, c


def _logits(rng, shape_nhwc, ties):
    n, h, w, c = shape_nhwc
    if ties:   # a few small integers: most pixels have an exact tie for the maximum
        return rng.integers(-1, 2, size=shape_nhwc).astype(np.float32)
    return rng.standard_normal(shape_nhwc).astype(np.float32)


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "gaussian"])
@pytest.mark.parametrize("classes", [1, 3, 4, 8, 11, 12, 16])
def test_logits_match_update_on_the_argmax(classes, ties):
    E = _E()
    n, h, w = 2, 19, 150
    rng = np.random.default_rng(seed("logits", classes, ties))
    lg = _logits(rng, (n, h, w, classes), ties)
    t = rng.integers(0, classes, size=(n, h, w))
    t[rng.random(t.shape) < 0.1] = -100
    for tdt in (torch.int64, torch.uint8):
        ign = -100 if tdt == torch.int64 else 156                # -100 as a uint8
        dt = _dev(t, tdt)
        forms = {
            "nhwc_f32": (torch.from_numpy(lg).cuda(), "nhwc", 3),
            "nhwc_bf16": (torch.from_numpy(lg).cuda().to(torch.bfloat16), "nhwc", 3),
            "nchw_f32": (torch.from_numpy(lg).cuda().permute(0, 3, 1, 2).contiguous(), "nchw", 1),
        }
        # the same NHWC logits one element into a longer buffer: no 16-byte loads there
        for name in ("nhwc_f32", "nhwc_bf16"):
            src = forms[name][0]
            buf = torch.empty(src.numel() + 1, dtype=src.dtype, device="cuda")
            buf[1:].copy_(src.reshape(-1))
            forms[name + "_offset"] = (buf[1:].view(src.shape), "nhwc", 3)
        for name, (dl, layout, axis) in forms.items():
            a = E.SegEvaluator(classes, ignore_index=ign).update_logits(dt, dl, layout)
            b = E.SegEvaluator(classes, ignore_index=ign).update(dt, dl.float().argmax(axis))
            np.testing.assert_array_equal(_state(a), _state(b), err_msg=name)
            vals = dl.float().cpu().numpy()                      # bf16 rounding can create ties: the restatement sees them
            ref = R.eval_state(dt.cpu().numpy(), R.argmax_first(vals, axis), classes, ign)
            np.testing.assert_array_equal(_state(a), ref, err_msg=name)


def test_logits_nan_beats_everything_like_predict():
    E = _E()
    rng = np.random.default_rng(5)
    lg = rng.standard_normal((1, 9, 70, 8)).astype(np.float32)
    lg[rng.random(lg.shape) < 0.05] = np.nan
    t = rng.integers(0, 8, size=(1, 9, 70))
    for dl in (torch.from_numpy(lg).cuda(), torch.from_numpy(lg).cuda().to(torch.bfloat16)):
        a = E.SegEvaluator(8).update_logits(_dev(t, torch.int64), dl, "nhwc")
        vals = dl.float().cpu().numpy()                          # as stored: bf16 rounding moves maxima and makes ties
        assert np.isnan(vals).sum() == np.isnan(lg).sum() > 0
        np.testing.assert_array_equal(_state(a), R.eval_state(t, R.argmax_first(vals, 3), 8))


def _unet():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    return UNet(1, 8, init_features=4), (2, 1, 32, 32)


def _bionet():
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet import BioUNet
    return BioUNet(1, 2), (1, 1, 16, 16)


def _mgunet2():
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    return M.MGUNet_2(1, 3, feature_scale=16), (2, 1, 48, 64)


@pytest.mark.parametrize("make", [_unet, _bionet, _mgunet2], ids=["UNet", "BioUNet", "MGUNet_2"])
def test_update_model_equals_update_on_predict(make):
    E = _E()
    torch.manual_seed(3)
    model, xs = make()
    model = model.cuda().eval()
    classes = model._classes() if hasattr(model, "_classes") else model._engine.ncls
    g = torch.Generator().manual_seed(4)
    x = torch.randn(*xs, generator=g).cuda()
    t = torch.randint(0, classes, (xs[0],) + xs[2:], generator=g)
    t[torch.rand(t.shape, generator=g) < 0.1] = 255
    t = t.to(torch.uint8).cuda()
    a = E.SegEvaluator(classes, ignore_index=255).update_model(model, x, t)
    pred = model.predict(x)
    b = E.SegEvaluator(classes, ignore_index=255).update(t, pred)
    np.testing.assert_array_equal(_state(a), _state(b))
    np.testing.assert_array_equal(_state(a), R.eval_state(t.cpu().numpy(), pred.cpu().numpy(), classes, 255))
    assert a.compute()["n"] + a.compute()["ignored"] == t.numel()


# ---- two ranks over gloo on the one GPU -----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_data():
    rng = np.random.default_rng(21)
    return R.layered_maps(rng, (5, 33, 130), 8)                  # 5 images: shards of 3 and 2


def _worker(rank, world, port, out_dir):
    import datetime
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp, evaluation
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    t, p = _rank_data()
    lo, hi = ddp.shard_batch(t.shape[0], rank, world)
    ev = evaluation.SegEvaluator(8)
    ev.update(torch.from_numpy(t[lo:hi]).cuda(), torch.from_numpy(p[lo:hi]).cuda())
    local = ev.state.cpu().numpy().copy()
    ev.all_reduce()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), state=ev.state.cpu().numpy(), local=local, lo=lo, hi=hi)
    dist.destroy_process_group()


def test_two_ranks_all_reduce_to_the_single_process_state(tmp_path):
    E = _E()
    world = 2
    ctx = mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=False)
    deadline = time.monotonic() + 180                            # a guard for every child, not a wait: join returns at exit
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("a rank did not finish within 180 s")
    t, p = _rank_data()
    single = _state(E.SegEvaluator(8).update(_dev(t, torch.int64), _dev(p, torch.int64)))
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["lo"]) == 0 and int(r0["hi"]) == int(r1["lo"]) and int(r1["hi"]) == 5
    np.testing.assert_array_equal(r0["state"], r1["state"])
    np.testing.assert_array_equal(r0["local"] + r1["local"], r0["state"])
    want = single.copy()
    want[-1] = 2                                                 # two updates, one per rank
    np.testing.assert_array_equal(r0["state"], want)
    np.testing.assert_array_equal(r0["state"], R.eval_state(t[:int(r0["hi"])], p[:int(r0["hi"])], 8)
                                  + R.eval_state(t[int(r1["lo"]):], p[int(r1["lo"]):], 8))
