"""GPU: the score evaluator (csrc/score_eval.hip, evaluation.ScoreEvaluator, auc_score) against the int64 restatement
tests/score_ref.py.  Every comparison on states and counts is on integers and exact; compute() is compared with == against
score_metrics_from_state on the restatement's state.  Shapes are the smallest at which the kernel can go wrong: one element,
odd tails (element-wise loads), 16 channels, and 90 000 elements of one channel -- more than a 16-bit packed counter holds
between two flushes, with a constant field putting all of them into one bin.  Two shapes more than the minimum, one per path
of the kernel that the others leave out: 2 x 3 x 8 x 12 takes the 4-element loads with several channels and less than one
step of a workgroup, 1 x 1 x 251 x 251 the element-wise loads over two tiles of one plane."""
import functools
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import score_ref as R
from oracle.bounds import Out, seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 33, 130), (2, 16, 9, 70), (1, 1, 300, 300), (2, 3, 8, 12), (1, 1, 251, 251)]
FIELDS = ("smooth", "random", "special")
_ID = lambda s: "x".join(map(str, s))  # noqa: E731


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


@functools.lru_cache(maxsize=None)
def _field(shape, kind, ignore):
    """(target uint8, scores fp32, bf16-valued scores, reference states for both): computed once per case, never modified"""
    rng = np.random.default_rng(seed(shape, kind, ignore))
    if kind == "smooth":
        t, s = R.smooth_field(rng, shape)
    elif kind == "random":
        t, s = R.random_field(rng, shape)
    elif kind == "special":
        t, s = R.special_field(rng, shape)
    else:
        t, s = R.constant_field(shape, -3.0, int(kind[-1]))
    if ignore is not None:
        t = t.copy()
        t[rng.random(shape) < 0.25] = ignore
    sb = R.to_bf16_values(s)
    ch = shape[1]
    out = (t, s, sb, R.score_state(t, s, ch, ignore), R.score_state(t, sb, ch, ignore))
    for a in out:
        a.setflags(write=False)
    return out


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _state(ev):
    return ev.state.cpu().numpy()


def _eq(got, ref, what):
    np.testing.assert_array_equal(got, ref, err_msg=what)


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_state_matches_the_restatement_in_every_form(shape, kind):
    E = _E()
    ch = shape[1]
    for ignore in (None, 255):
        t, s, sb, ref, ref_b = _field(shape, kind, ignore)
        dt, ds = _dev(t), _dev(s)
        forms = {
            "nchw_f32": (ds, "nchw", ref),
            "nhwc_f32": (ds.permute(0, 2, 3, 1).contiguous(), "nhwc", ref),
            "nhwc_bf16": (ds.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous(), "nhwc", ref_b),
            "flat_bf16": (ds.to(torch.bfloat16), "nchw", ref_b),
        }
        for name, (sc, layout, want) in forms.items():
            ev = E.ScoreEvaluator(ch, ignore_value=ignore).update(dt, sc, layout)
            got = _state(ev)
            _eq(got, want, f"{kind} {name} ignore {ignore}")
    # the bf16 tensor holds what the restatement rounded: the two references describe the same device values
    assert np.array_equal(ds.to(torch.bfloat16).float().cpu().numpy(), sb, equal_nan=True)


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_uint8_scores_match_the_restatement(shape):
    E = _E()
    rng = np.random.default_rng(seed("u8", shape))
    s8 = rng.integers(0, 256, size=shape).astype(np.uint8)
    t = (s8.astype(np.float32) + 60.0 * rng.standard_normal(shape) > 128).astype(np.uint8)
    for ignore in (None, 255):
        tt = t.copy()
        if ignore is not None:
            tt[rng.random(shape) < 0.25] = ignore
        ev = E.ScoreEvaluator(shape[1], ignore_value=ignore, logits=False).update(_dev(tt), _dev(s8))
        _eq(_state(ev), R.score_state(tt, s8.astype(np.float32), shape[1], ignore), f"uint8 ignore {ignore}")
    b = (s8 > 100)                                                               # bool scores are 0 / 1 uint8 scores
    ev = E.ScoreEvaluator(shape[1], logits=False).update(_dev(t).bool(), _dev(b))
    _eq(_state(ev), R.score_state(t, b.astype(np.float32), shape[1]), "bool")


@pytest.mark.parametrize("label", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 300, 300), (2, 3, 5, 7), (1, 1, 251, 251)], ids=_ID)
def test_constant_field_lands_in_one_bin(shape, label):
    """the maximum-conflict case: every lane of every wave adds to one packed counter, 90 000 times at the larger shape"""
    E = _E()
    t, s, _, ref, _ = _field(shape, f"constant{label}", None)
    for sc in (_dev(s), _dev(s).to(torch.bfloat16)):                             # -3 is on the bf16 grid
        got = _state(E.ScoreEvaluator(shape[1]).update(_dev(t), sc))
        _eq(got, ref, "constant")
        k = int(R.key16(np.float32(-3.0)))
        per = shape[0] * shape[2] * shape[3]
        assert got[label * R.KEYS + k] == per and got[:shape[1] * 2 * R.KEYS].sum() == per * shape[1]


def test_a_label_of_two_without_ignore_value_lands_in_invalid_and_nothing_is_written_outside():
    E = _E()
    shape = (2, 3, 33, 130)
    rng = np.random.default_rng(seed("invalid"))
    t, s = R.random_field(rng, shape)
    t = t.copy()
    bad = rng.random(shape) < 0.07
    t[bad] = rng.choice([2, 3, 200, 255], size=int(bad.sum()))
    ref = R.score_state(t, s, 3)
    nh = 3 * 2 * R.KEYS
    assert ref[nh + 6:nh + 9].sum() == int(bad.sum()) > 0 and ref[nh + 3:nh + 6].sum() == 0
    out = Out((E.score_state_size(3),), torch.int64, fill=-7777)
    out.t.zero_()
    ev = E.ScoreEvaluator(3)
    ev.state = out.t
    ev.update(_dev(t), _dev(s))
    got = out.host()                                                             # asserts the sentinel tail
    _eq(got, ref, "invalid")
    assert got[:nh].sum() == int((~bad).sum())


def test_non_contiguous_and_misaligned_views():
    E = _E()
    shape = (2, 2, 9, 70)
    t, s, sb, ref, ref_b = _field(shape, "random", None)
    dt, ds = _dev(t), _dev(s)
    # non-contiguous: the NCHW values seen through a permuted NHWC buffer, and a strided target
    nc = ds.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    tn = torch.stack([dt, dt], dim=-1)[..., 0]
    assert not nc.is_contiguous() and not tn.is_contiguous()
    _eq(_state(E.ScoreEvaluator(2).update(tn, nc)), ref, "non-contiguous")
    # bf16 scores one element (2 bytes) into a longer buffer, the target one byte into its own: no 4-element loads
    src = ds.to(torch.bfloat16)
    buf = torch.empty(src.numel() + 1, dtype=torch.bfloat16, device="cuda")
    buf[1:].copy_(src.reshape(-1))
    tb = torch.empty(dt.numel() + 1, dtype=torch.uint8, device="cuda")
    tb[1:].copy_(dt.reshape(-1))
    vs, vt = buf[1:].view(shape), tb[1:].view(shape)
    assert vs.data_ptr() % 4 == 2 and vt.data_ptr() % 2 == 1
    _eq(_state(E.ScoreEvaluator(2).update(vt, vs)), ref_b, "misaligned both")
    _eq(_state(E.ScoreEvaluator(2).update(dt, vs)), ref_b, "misaligned scores")
    _eq(_state(E.ScoreEvaluator(2).update(vt, src)), ref_b, "misaligned target")
    # a (B, H, W) pair for one channel
    t1, s1, _, ref1, _ = _field((2, 1, 9, 70), "smooth", None)
    _eq(_state(E.ScoreEvaluator(1).update(_dev(t1)[:, 0], _dev(s1)[:, 0])), ref1, "3-D")


def test_updates_accumulate_without_a_synchronisation_reset_zeroes_and_zero_images_count():
    E = _E()
    a, b = _field((2, 3, 5, 7), "random", 255), _field((2, 3, 5, 7), "smooth", 255)
    dev = [(_dev(c[0]), _dev(c[1])) for c in (a, b)]
    ev = E.ScoreEvaluator(3, ignore_value=255)
    ev.update(*dev[0]).reset()                                                   # state allocated, then zero
    assert not _state(ev).any()
    empty_t = torch.empty((0, 3, 5, 7), dtype=torch.uint8, device="cuda")
    empty_s = torch.empty((0, 3, 5, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t, s in dev:
            ev.update(t, s)
        ev.update(empty_t, empty_s)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    want = a[3] + b[3]
    want[-1] = 3                                                                 # the zero-image update counts as a call
    _eq(_state(ev), want, "two updates + an empty one")
    assert ev.compute()["updates"] == 3
    ev.reset()
    assert not _state(ev).any() and ev.compute()["updates"] == 0
    assert E.ScoreEvaluator(3).compute()["updates"] == 0                         # before any update: no state, no launch


def _same_metrics(got, want):
    assert got.keys() == want.keys()
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert ((a == b) | (np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)))).all(), k


@pytest.mark.parametrize("shape,kind", [((1, 2, 33, 130), "random"), ((2, 16, 9, 70), "smooth"), ((2, 3, 5, 7), "special")])
def test_compute_equals_the_numpy_function_on_the_restatement_state(shape, kind):
    E = _E()
    t, s, _, ref, _ = _field(shape, kind, 255)
    ev = E.ScoreEvaluator(shape[1], ignore_value=255).update(_dev(t), _dev(s))
    ths = (0.5, 0.3, 0.8)
    _same_metrics(ev.compute(thresholds=ths), E.score_metrics_from_state(ref, shape[1], ths, True))
    want = E.score_curves_from_state(ref, shape[1], shape[1] - 1)
    fpr, tpr, thr = ev.roc_curve(shape[1] - 1)
    prec, rec, thr2 = ev.pr_curve(shape[1] - 1)
    _same_metrics({"fpr": fpr, "tpr": tpr, "thr": thr, "prec": prec, "rec": rec, "thr2": thr2},
                  {"fpr": want["fpr"], "tpr": want["tpr"], "thr": want["thresholds"], "prec": want["precision"],
                   "rec": want["tpr"], "thr2": want["thresholds"]})


# ---- against the head itself --------------------------------------------------------------------------------------------------
def _counts_of(mask, t, keep=None):
    """tp, t, p, tn, fp, fn per channel of a bool prediction (B, C, H, W) against a uint8 target, over the kept elements"""
    keep = torch.ones_like(mask) if keep is None else keep
    pos, neg = (t == 1) & keep, (t == 0) & keep
    f = lambda x: x.sum(dim=(0, 2, 3)).cpu().numpy()  # noqa: E731
    return np.stack([f(mask & pos), f(pos), f(mask & keep), f(~mask & neg), f(mask & neg), f(~mask & pos)], axis=1)


def test_engine_network_counts_equal_the_logits_and_predict_mask():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd.unet3d import UNet3D
    E = _E()
    torch.manual_seed(3)
    model = UNet(1, 2, init_features=4).cuda().eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 1, 32, 32, generator=g).cuda()
    t = (torch.rand(1, 2, 32, 32, generator=g) < 0.4).to(torch.uint8).cuda()
    lg = model.logits(x)
    assert lg.shape == (1, 2, 32, 32) and lg.dtype == torch.float32
    a = E.ScoreEvaluator(2).update(t, lg)
    m = a.compute(thresholds=(0.5,))
    np.testing.assert_array_equal(m["counts"][:, 0], _counts_of(lg >= 0, t))
    np.testing.assert_array_equal(m["counts"][:, 0], _counts_of(model.predict_mask(x).bool(), t))
    b = E.ScoreEvaluator(2).update_model(model, x, t)
    _eq(_state(b), _state(a), "update_model")
    _eq(_state(b), R.score_state(t.cpu().numpy(), lg.cpu().numpy(), 2), "update_model vs restatement")
    with pytest.raises(NotImplementedError):
        E.ScoreEvaluator(2).update_model(UNet3D(1, 2, init_features=4).cuda().eval(), torch.zeros(1, 1, 4, 16, 16).cuda(),
                                         torch.zeros(1, 2, 4, 16, 16, dtype=torch.uint8).cuda())
    with pytest.raises(RuntimeError, match="output channels"):
        E.ScoreEvaluator(3).update_model(model, x, t)


def test_logits_network_goes_the_nhwc_route():
    from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment import MGUNet_2021 as M
    E = _E()
    torch.manual_seed(3)
    model = M.MGUNet_2(1, 3, feature_scale=16).cuda().eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 1, 48, 64, generator=g).cuda()
    t = (torch.rand(2, 3, 48, 64, generator=g) < 0.4).to(torch.uint8)
    t[torch.rand(t.shape, generator=g) < 0.1] = 255
    t = t.cuda()
    with torch.no_grad():
        nchw = model(x)                                                          # the same logits as (B, C, H, W) fp32
    a = E.ScoreEvaluator(3, ignore_value=255).update_model(model, x, t)
    b = E.ScoreEvaluator(3, ignore_value=255).update(t, nchw)
    _eq(_state(a), _state(b), "update_model vs update on forward()")
    _eq(_state(a), R.score_state(t.cpu().numpy(), nchw.cpu().numpy(), 3, 255), "update_model vs restatement")
    m = a.compute(thresholds=(0.5,))
    np.testing.assert_array_equal(m["counts"][:, 0], _counts_of(nchw >= 0, t, t != 255))
    np.testing.assert_array_equal(m["counts"][:, 0], _counts_of(model.predict_mask(x).bool(), t, t != 255))


# ---- CM.auc_score ------------------------------------------------------------------------------------------------------
def test_auc_score_on_the_device_where_it_is_exact_and_on_the_host_otherwise():
    from retinal_oct_image_segmentation_via_deep_learning_amd.Metrics import ConfusionMatrix_based_metrics as CM
    E = _E()
    shape = (1, 1, 33, 130)
    t, s, sb, ref, ref_b = _field(shape, "random", None)
    dt = _dev(t)
    # bf16 pair
    got = CM.auc_score(dt, _dev(s).to(torch.bfloat16))
    want = E.score_metrics_from_state(ref_b, 1)["auc"][0]
    assert isinstance(got, np.float64) and abs(got - want) <= 1e-12
    # uint8 pair (and a bool target)
    rng = np.random.default_rng(9)
    s8 = np.clip(128 + 20 * s + 10 * rng.standard_normal(shape), 0, 255).astype(np.uint8)
    want8 = E.score_metrics_from_state(R.score_state(t, s8.astype(np.float32), 1), 1)["auc"][0]
    assert abs(CM.auc_score(dt, _dev(s8)) - want8) <= 1e-12
    assert abs(CM.auc_score(dt.bool(), _dev(s8)) - want8) <= 1e-12
    # everything else is the present host code: fp32 device pair, numpy pair
    assert CM._auc_on_device(dt, _dev(s)) is None and CM._auc_on_device(t, s) is None
    assert CM.auc_score(dt, _dev(s)) == CM._auc_on_host(dt, _dev(s))
    assert CM.auc_score(t.ravel(), s.ravel()) == CM._auc_on_host(t.ravel(), s.ravel())
    # the edge cases stay sklearn's: one class only is answered by the host route (0.0 or NaN, as sklearn decides), for bf16 too
    ones = torch.ones_like(dt)
    assert CM._auc_on_device(ones, _dev(s).to(torch.bfloat16)) is None
    a, b = CM.auc_score(ones, _dev(s).to(torch.bfloat16)), CM._auc_on_host(ones, _dev(s))
    assert a == b or (np.isnan(a) and np.isnan(b))
    # where both run, the device value is sklearn's
    assert abs(got - CM._auc_on_host(dt, _dev(s).to(torch.bfloat16))) <= 1e-12


# ---- error paths --------------------------------------------------------------------------------------------------------------
def test_update_refuses_what_it_cannot_score():
    E = _E()
    ev = E.ScoreEvaluator(2)
    t = torch.zeros(1, 2, 4, 6, dtype=torch.uint8, device="cuda")
    s = torch.zeros(1, 2, 4, 6, device="cuda")
    with pytest.raises(RuntimeError, match="channels"):
        ev.update(torch.zeros(1, 3, 4, 6, dtype=torch.uint8, device="cuda"), torch.zeros(1, 3, 4, 6, device="cuda"))
    with pytest.raises(RuntimeError, match="shape"):
        ev.update(t[:, :, :3], s)
    with pytest.raises(RuntimeError, match="4-D"):
        ev.update(t, s[0, 0])
    with pytest.raises(RuntimeError, match="uint8 or bool"):
        ev.update(t.long(), s)
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(RuntimeError, match="fp32, bf16 or uint8"):
            ev.update(t, s.to(bad))
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        ev.update(t, torch.zeros(1, 4, 6, 2, dtype=torch.uint8, device="cuda"), "nhwc")
    with pytest.raises(ValueError, match="layout"):
        ev.update(t, s, "chwn")
    with pytest.raises(RuntimeError, match="is on"):
        ev.update(t.cpu(), s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(t.cpu(), s.cpu())
    with pytest.raises(TypeError):
        ev.update(t, s.cpu().numpy())
    # 2^31 elements: refused before anything is made contiguous (the views below own one byte / four bytes)
    big_t = torch.zeros(1, dtype=torch.uint8, device="cuda").expand(1, 2, 32768, 32768)
    big_s = torch.zeros(1, device="cuda").expand(1, 2, 32768, 32768)
    with pytest.raises(RuntimeError, match="2\\^31"):
        ev.update(big_t, big_s)
    assert ev.state is None                                                      # nothing was launched or allocated


def test_the_library_checks_its_descriptor():
    import ctypes as C
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    lib = L.lib()
    assert lib.oct_score_eval_state_elems(3) == 3 * (2 * 65536 + 3) + 1
    assert lib.oct_score_eval_state_elems(0) == 0 and lib.oct_score_eval_state_elems(17) == 0
    st = torch.zeros(2 * 65536 + 4, dtype=torch.int64, device="cuda")
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for desc, what in ((L.ScoreEvalDesc(1, 4, 4, 0, 0, 0, 0), "channels"), (L.ScoreEvalDesc(1, 4, 4, 17, 0, 0, 0), "channels"),
                       (L.ScoreEvalDesc(1, 0, 4, 1, 0, 0, 0), "geometry"), (L.ScoreEvalDesc(-1, 4, 4, 1, 0, 0, 0), "geometry"),
                       (L.ScoreEvalDesc(2, 32768, 32768, 1, 0, 0, 0), "2^31"), (L.ScoreEvalDesc(1, 4, 4, 1, 3, 0, 0), "scores are"),
                       (L.ScoreEvalDesc(1, 4, 4, 1, 0, 1, 1), "ignore_value")):
        assert lib.oct_score_eval_update(C.byref(desc), buf.data_ptr(), buf.data_ptr(), st.data_ptr(), None) == -22
        assert what in L.last_error(), (what, L.last_error())
    assert lib.oct_score_eval_update(C.byref(L.ScoreEvalDesc(1, 4, 4, 1, 0, 0, 0)), None, buf.data_ptr(), st.data_ptr(), None) == -22
    assert lib.oct_score_eval_update(C.byref(L.ScoreEvalDesc(1, 4, 4, 1, 0, 0, 0)), buf.data_ptr(), buf.data_ptr() + 2, st.data_ptr(),
                                     None) == -22 and "aligned" in L.last_error()
    torch.cuda.synchronize()
    assert not st.any()


# ---- two ranks over gloo on the one GPU -----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_data():
    rng = np.random.default_rng(21)
    return R.smooth_field(rng, (5, 2, 33, 130))                                  # 5 images: shards of 3 and 2


def _worker(rank, world, port, out_dir):
    import datetime
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp, evaluation
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    t, s = _rank_data()
    lo, hi = ddp.shard_batch(t.shape[0], rank, world)
    ev = evaluation.ScoreEvaluator(2)
    ev.update(torch.from_numpy(t[lo:hi]).cuda(), torch.from_numpy(s[lo:hi]).cuda())
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
    t, s = _rank_data()
    single = _state(E.ScoreEvaluator(2).update(_dev(t), _dev(s)))
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["lo"]) == 0 and int(r0["hi"]) == int(r1["lo"]) and int(r1["hi"]) == 5
    np.testing.assert_array_equal(r0["state"], r1["state"])
    np.testing.assert_array_equal(r0["local"] + r1["local"], r0["state"])
    want = single.copy()
    want[-1] = 2                                                 # two updates, one per rank
    np.testing.assert_array_equal(r0["state"], want)
    np.testing.assert_array_equal(r0["state"], R.score_state(t[:int(r0["hi"])], s[:int(r0["hi"])], 2)
                                  + R.score_state(t[int(r1["lo"]):], s[int(r1["lo"]):], 2))
