"""CPU: the layer-surface restatement (tests/surf_ref.py) against a brute force over all paths with the stated tie order, on
known answers and on the properties the design claims (ordered minimisers, the ordinal L1 objective, smoothing helps on noise);
surface_metrics_from_state on hand-made states; the argument errors of surfaces.py / SurfaceEvaluator and the C-ABI refusals
without a GPU.  Everything is an integer: every comparison of surfaces, maps and costs is ==."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import surf_ref as R


@pytest.fixture(scope="module")
def L():
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


def _S():
    from retinal_oct_image_segmentation_via_deep_learning_amd import surfaces
    return surfaces


def _E():
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation
    return evaluation


# ---- the restatement against all paths ------------------------------------------------------------------------------------------
def _brute(u, max_step):
    """[K-1, W] by enumeration: among the feasible paths of least cost the one that is smallest read from the LAST column back
    (what 'smallest argmin of the last column, then the smallest t' selects), then the running maximum; the costs too"""
    K, H, W = u.shape
    out, costs = [], []
    for k in range(1, K):
        d = [[min(int(u[j, y, x]) for j in range(k)) - min(int(u[j, y, x]) for j in range(k, K)) for x in range(W)] for y in range(H)]
        best = None
        for path in itertools.product(range(H + 1), repeat=W):
            if max_step is not None and any(abs(path[x + 1] - path[x]) > max_step for x in range(W - 1)):
                continue
            cost = sum(d[y][x] for x in range(W) for y in range(path[x]))
            key = (cost, path[::-1])
            if best is None or key < best:
                best = key
        out.append(best[1][::-1])
        costs.append(best[0])
    return np.maximum.accumulate(np.array(out, dtype=np.int32), axis=0), costs


def test_restatement_equals_brute_force_over_all_paths():
    rng = np.random.default_rng(11)
    checked = 0
    for H, W, K in itertools.product((1, 2, 3, 4), (1, 2, 3, 4), (2, 3)):
        for trial in range(3):
            if trial < 2:      # maps: classes 0..K-1 in a scrambled order, class K (not in order) and an out-of-range value: free
                order = list(rng.permutation(K))
                m = rng.integers(0, K + 2, size=(H, W))
                u = R.unary_map(m, order, K + 1)
            else:              # scores with few distinct values: many ties
                order = list(rng.permutation(K + 1)[:K])
                z = rng.integers(-2, 3, size=(K + 1, H, W)).astype(np.float32) / 4
                u = R.unary_scores(z, order, scale=2.0, qmax=3)
            for step in (None, 0, 1, 2):
                want, costs = _brute(u, step)
                np.testing.assert_array_equal(R.surfaces_from_unary(u, step), want, err_msg=f"{H}x{W} K={K} step={step}\n{u}")
                N = R.path_costs(u)
                assert [R.shortest_path(N[k], step)[1] for k in range(K - 1)] == costs
                checked += 1
    assert checked == 4 * 4 * 2 * 3 * 4


def _wavy_cuts(rng, h, w, k, step):
    """int [k-1, w]: ordered cuts that move at most `step` rows per column"""
    base = np.sort(rng.integers(2, h - 2, size=k - 1))
    walk = np.cumsum(rng.integers(-step, step + 1, size=(k - 1, w)), axis=1) if step else np.zeros((k - 1, w), dtype=np.int64)
    cuts = np.clip(base[:, None] + walk, 0, h)
    for _ in range(4 * w):      # clipping and ordering may have made steps too long: pull them in until none is
        cuts = np.maximum.accumulate(cuts, axis=0)
        for x in range(1, w):
            cuts[:, x] = np.clip(cuts[:, x], cuts[:, x - 1] - step, cuts[:, x - 1] + step)
        if (np.diff(cuts, axis=0) >= 0).all() and (np.abs(np.diff(cuts, axis=1)) <= step).all():
            return cuts
    raise AssertionError("no valid cuts")


def test_valid_band_map_comes_back_exactly_and_paints_to_itself():
    rng = np.random.default_rng(3)
    for h, w, k, step in ((20, 31, 4, 1), (48, 64, 5, 2), (9, 7, 2, 0), (30, 40, 6, 3)):
        cuts = _wavy_cuts(rng, h, w, k, step)
        m = R.band_map(h, w, cuts)
        order = list(range(k))
        for ms in (step, None, 32):
            s = R.extract(m, order, k, max_step=ms)
            np.testing.assert_array_equal(s, cuts.astype(np.int32), err_msg=f"{h}x{w} k={k} step={ms}")
            np.testing.assert_array_equal(R.paint(s, order, h), m)
    # a scrambled class numbering, a kept class inside a band and ignored pixels change nothing
    order, cuts = [3, 0, 2], np.array([[2, 3, 3, 4], [6, 6, 7, 7]])
    m = np.asarray(order)[R.band_map(9, 4, cuts)]
    noisy = m.copy()
    noisy[4, 1], noisy[0, 0] = 1, 4      # class 1 is kept (fluid), 4 is the ignore_index
    s = R.extract(noisy, order, 5, max_step=1, ignore_index=4)
    np.testing.assert_array_equal(s, cuts.astype(np.int32))
    painted = R.paint(s, order, 9, keep=(1,), input_classes=noisy)
    assert painted[4, 1] == 1 and painted[0, 0] == order[0]
    painted[4, 1] = m[4, 1]
    np.testing.assert_array_equal(painted, m)


def _noisy_bands(seed, h=48, w=64, k=5, flip=0.3):
    rng = np.random.default_rng(seed)
    cuts = _wavy_cuts(rng, h, w, k, 1)
    clean = R.band_map(h, w, cuts)
    noisy = np.where(rng.random((h, w)) < flip, rng.integers(0, k, size=(h, w)), clean)
    return cuts, clean, noisy


def test_raw_minimisers_are_ordered_and_the_objective_is_the_ordinal_l1_distance():
    k = 5
    for seed in range(6):
        _, _, noisy = _noisy_bands(100 + seed)
        if seed % 2:
            noisy[np.random.default_rng(seed).random(noisy.shape) < 0.1] = k      # free pixels
        u = R.unary_map(noisy, range(k), k + 1)
        N = R.path_costs(u)
        for step in (None, 0, 1, 3):
            raw = R.surfaces_from_unary(u, step, raw=True)
            assert (np.diff(raw.astype(np.int64), axis=0) >= 0).all(), f"seed {seed} step {step}: the minimisers cross"
            s = R.surfaces_from_unary(u, step)
            np.testing.assert_array_equal(s, raw)      # so the running maximum changes nothing
            cost = sum(int(N[i, np.arange(N.shape[1]), s[i]].sum()) for i in range(k - 1))
            assert cost == sum(R.shortest_path(N[i], step)[1] for i in range(k - 1))
            painted = R.paint(s, list(range(k)), noisy.shape[0])
            live = noisy < k
            constant = int((k - 1 - noisy[live]).sum())      # sum over the pixels of #{k : position < k}
            assert cost + constant == int(np.abs(painted - noisy)[live].sum()), f"seed {seed} step {step}"


def test_smoothing_lowers_the_surface_error_on_label_noise():
    """48 x 64, K = 5, 30 % of the labels replaced uniformly at random: this seeded case gives a mean absolute surface error of
    0.43 px with max_step = 1 against 0.89 px with max_step = None (the figures the test prints)"""
    cuts, _, noisy = _noisy_bands(2024)
    err = {step: float(np.abs(R.extract(noisy, range(5), 5, max_step=step).astype(np.int64) - cuts).mean()) for step in (1, None)}
    print("mean absolute surface error:", err)
    assert err[1] < err[None]


def test_scores_unary_on_known_values():
    z = np.array([[0.0], [1.0], [np.inf], [-np.inf]], dtype=np.float32).reshape(4, 1, 1)
    np.testing.assert_array_equal(R.unary_scores(z, [0, 1, 2, 3], 16.0, 255).ravel(), [255, 255, 0, 255])
    z = np.array([0.0, -0.03, -0.04, -1.0, -15.9, -16.0], dtype=np.float32).reshape(6, 1, 1)      # 16 * 0.03 + 0.5 = 0.98
    np.testing.assert_array_equal(R.unary_scores(z, range(6), 16.0, 255).ravel(), [0, 0, 1, 16, 254, 255])
    np.testing.assert_array_equal(R.unary_scores(z, range(6), 16.0, 1).ravel(), [0, 0, 1, 1, 1, 1])
    z = np.array([0.0, np.nan, 3.0], dtype=np.float32).reshape(3, 1, 1)
    np.testing.assert_array_equal(R.unary_scores(z, [0, 2], 16.0, 255).ravel(), [0, 0])      # a NaN anywhere frees the pixel
    assert R.argmax_first(z).item() == 1 and R.argmax_first(z[::-1]).item() == 1
    assert R.argmax_first(np.zeros((3, 1, 1), np.float32)).item() == 0


# ---- the host half of the evaluator -----------------------------------------------------------------------------------------------
def test_surface_metrics_from_state_on_hand_made_states():
    E = _E()
    m = E.surface_metrics_from_state(np.array([[4, 6, -2, 14, 3], [0, 0, 0, 0, 0], [2, 0, 0, 0, 0]], dtype=np.int64), 3)
    np.testing.assert_array_equal(m["columns"], [4, 0, 2])
    np.testing.assert_array_equal(m["mean_abs_error"], [1.5, np.nan, 0.0])
    np.testing.assert_array_equal(m["mean_signed_error"], [-0.5, np.nan, 0.0])
    np.testing.assert_array_equal(m["rmse"], [np.sqrt(3.5), np.nan, 0.0])
    np.testing.assert_array_equal(m["max_abs_error"], [3.0, np.nan, 0.0])
    assert m["mean_mean_abs_error"] == 0.75 and m["mean_mean_signed_error"] == -0.25
    assert m["mean_rmse"] == np.sqrt(3.5) / 2 and m["mean_max_abs_error"] == 1.5
    empty = E.surface_metrics_from_state(np.zeros(10, dtype=np.int64), 2)
    assert np.isnan(empty["mean_abs_error"]).all() and np.isnan(empty["mean_rmse"]) and empty["columns"].tolist() == [0, 0]
    # the state of the restatement: e = [1, -3, 0, 2] and [0, 0, 0, 0]
    t = np.array([[[5, 5, 5, 5], [7, 7, 7, 7]]], dtype=np.int32)
    p = np.array([[[6, 2, 5, 7], [7, 7, 7, 7]]], dtype=np.int32)
    np.testing.assert_array_equal(R.error_state(t, p), [[4, 6, 0, 14, 3], [4, 0, 0, 0, 0]])
    np.testing.assert_array_equal(R.error_state(t, p, np.array([[1, 0, 1, 1]])), [[3, 3, 3, 5, 2], [3, 0, 0, 0, 0]])
    for bad, exc in ((np.zeros(9, np.int64), ValueError), (np.zeros(10, np.float64), ValueError)):
        with pytest.raises(exc):
            E.surface_metrics_from_state(bad, 2)
    with pytest.raises(ValueError):
        E.surface_metrics_from_state(np.zeros(0, np.int64), 0)
    assert E.SurfaceEvaluator(3).compute()["columns"].tolist() == [0, 0, 0]      # before the first update: zeros, no GPU needed


# ---- argument errors, before anything is launched -----------------------------------------------------------------------------------
def test_constructor_refusals():
    LS = _S().LayerSurfaces
    for kw, exc in ((dict(order=[0]), ValueError), (dict(order=list(range(17)), classes=16), ValueError),
                    (dict(order=[0, 0, 1]), ValueError),
                    (dict(order=[0, 9]), ValueError), (dict(order=[0, -1]), ValueError), (dict(order="01"), TypeError),
                    (dict(order=[0, 1.0]), TypeError), (dict(order=[0, True]), TypeError), (dict(order=5), TypeError),
                    (dict(keep=[1]), ValueError), (dict(keep=[3, 3]), ValueError), (dict(keep=[9]), ValueError), (dict(keep=3), TypeError),
                    (dict(max_step=-1), ValueError), (dict(max_step=33), ValueError), (dict(max_step=1.0), TypeError),
                    (dict(max_step=True), TypeError), (dict(scale=0.0), ValueError), (dict(scale=-1.0), ValueError),
                    (dict(scale=float("inf")), ValueError), (dict(scale=float("nan")), ValueError), (dict(scale=1e39), ValueError),
                    (dict(scale=1e-50), ValueError), (dict(scale="16"), TypeError), (dict(scale=True), TypeError),
                    (dict(qmax=0), ValueError), (dict(qmax=256), ValueError), (dict(qmax=2.0), TypeError),
                    (dict(classes=0), ValueError), (dict(classes=17), ValueError), (dict(ignore_index=1.5), TypeError),
                    (dict(max_workspace_bytes=0), ValueError)):
        args = dict(classes=4, order=[0, 1, 2])
        args.update(kw)
        with pytest.raises(exc):
            LS(**args)
    ok = LS(4, range(3), max_step=None, keep=(3,), ignore_index=-1, scale=8, qmax=1)
    assert ok.order == [0, 1, 2] and ok.keep == [3] and ok.unconstrained() is ok
    smooth = LS(4, (2, 0, 1))
    assert smooth.max_step == 1 and smooth.unconstrained().max_step is None and smooth.unconstrained() is smooth.unconstrained()
    assert smooth.unconstrained().order == [2, 0, 1]


def test_input_refusals_and_the_int32_limit():
    LS = _S().LayerSurfaces
    ls = LS(3, [0, 1, 2])
    with pytest.raises(TypeError):
        ls.extract(np.zeros((4, 4), np.int64))
    with pytest.raises(TypeError):
        ls.extract(torch.zeros(4, 4))
    with pytest.raises(RuntimeError):
        ls.extract(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="H, W >= 1"):
        ls.extract(torch.zeros(2, 0, 4, dtype=torch.int64))
    with pytest.raises(TypeError):
        ls.extract_scores(torch.zeros(1, 3, 4, 4, dtype=torch.float16))
    with pytest.raises(TypeError):
        ls.extract_scores(torch.zeros(1, 3, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ls.extract_scores(torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="channels"):
        ls.extract_scores(torch.zeros(1, 4, 4, 4))
    # H > 4095 and qmax * H * W >= 2^31, on views that hold one element: the refusal comes before any copy
    one = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="H <= 4095"):
        ls.extract(one.expand(4096, 2))
    w = -(-2 ** 31 // 4095)
    with pytest.raises(RuntimeError, match="2\\^31"):
        ls.extract(one.expand(4095, w))
    with pytest.raises(RuntimeError, match="2\\^31"):
        ls.paint(one.expand(4095, w), torch.zeros(2, w, dtype=torch.int32))
    zero = torch.zeros(1)
    wq = -(-2 ** 31 // (255 * 4095))
    with pytest.raises(RuntimeError, match="2\\^31"):
        ls.extract_scores(zero.expand(1, 3, 4095, wq))
    with pytest.raises(_S().L.OctError, match="no CPU fallback"):      # just below the limit the check passes: the device rule is next
        LS(3, [0, 1, 2], qmax=1).extract_scores(zero.expand(1, 3, 2, 5))
    with pytest.raises(RuntimeError, match="H <= 4095"):
        ls.extract_scores(zero.expand(1, 3, 4096, 2))


def test_paint_and_evaluator_refusals():
    S, E = _S(), _E()
    ls = S.LayerSurfaces(3, [0, 1, 2])
    m = torch.zeros(2, 5, 7, dtype=torch.int64)
    for bad, exc in ((torch.zeros(2, 2, 7, dtype=torch.int64), TypeError), (torch.zeros(2, 3, 7, dtype=torch.int32), RuntimeError),
                     (torch.zeros(2, 2, 6, dtype=torch.int32), RuntimeError), (torch.zeros(1, 2, 7, dtype=torch.int32), RuntimeError),
                     (np.zeros((2, 2, 7), np.int32), TypeError)):
        with pytest.raises(exc):
            ls.paint(m, bad)
    with pytest.raises(S.L.OctError, match="no CPU fallback"):
        ls.paint(m, torch.zeros(2, 2, 7, dtype=torch.int32))
    for kw, exc in ((dict(surfaces=0), ValueError), (dict(surfaces=16), ValueError), (dict(surfaces=2.0), TypeError),
                    (dict(surfaces=2, device="cpu"), S.L.OctError)):
        with pytest.raises(exc):
            E.SurfaceEvaluator(**kw)
    ev = E.SurfaceEvaluator(2)
    t = torch.zeros(2, 2, 7, dtype=torch.int32)
    for args, exc in (((t.long(), t), TypeError), ((t, t.long()), TypeError), ((t, t[:, :, :6]), RuntimeError),
                      ((t[:, :1], t[:, :1]), RuntimeError),
                      ((t, t, torch.zeros(2, 7)), TypeError), ((t, t, torch.zeros(2, 6, dtype=torch.bool)), RuntimeError),
                      ((np.zeros((2, 2, 7)), t), TypeError)):
        with pytest.raises(exc):
            ev.update(*args)
    with pytest.raises(S.L.OctError, match="no CPU fallback"):
        ev.update(t, t)
    with pytest.raises(TypeError):
        ev.update_maps(m, m, None)
    with pytest.raises(RuntimeError, match="surfaces"):
        ev.update_maps(m, m, S.LayerSurfaces(4, [0, 1, 2, 3]))
    with pytest.raises(RuntimeError, match="same shape"):
        ev.update_maps(m, m[:1], ls)


def test_layer_surfaces_on_a_cpu_tensor_has_no_fallback():
    S = _S()
    ls = S.LayerSurfaces(3, [0, 1, 2], keep=())
    m = torch.zeros(1, 6, 8, dtype=torch.uint8)
    for call in (lambda: ls.extract(m), lambda: ls(m), lambda: ls.extract_scores(torch.zeros(1, 3, 6, 8)),
                 lambda: ls.unconstrained().extract(m)):
        with pytest.raises(S.L.OctError, match="no CPU fallback"):
            call()

    class Net:
        def logits(self, x):
            return torch.zeros(1, 3, 6, 8)

    with pytest.raises(S.L.OctError, match="no CPU fallback"):
        ls.from_model(Net(), None)
    with pytest.raises(TypeError):
        ls.from_model(object(), None)


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------------
def test_abi_workspace_formula_and_refusals(L):
    lib = L.lib()

    def desc(images=2, h=9, w=7, classes=4, elem=0, k=3, max_step=1, nkeep=0, qmax=255, scale=16.0):
        return L.SurfDesc(images, h, w, classes, elem, k, max_step, 0, nkeep, qmax, scale, 0, 0)

    def up(v):
        return (v + 255) // 256 * 256

    cells = 2 * 2 * 7 * 10
    assert lib.oct_surf_workspace_bytes(C.byref(desc())) == up(4 * cells) + up(cells)
    assert lib.oct_surf_workspace_bytes(C.byref(desc(max_step=-1))) == 0
    assert lib.oct_surf_workspace_bytes(C.byref(desc(images=32, h=512, w=1024, k=9))) == 5 * 32 * 8 * 1024 * 513
    order = (C.c_int32 * 3)(0, 1, 2)
    for d, msg in ((desc(h=4096), "h must not exceed"), (desc(k=1), "order must name"), (desc(k=17), "order must name"),
                   (desc(max_step=33), "max_step"), (desc(max_step=-2), "max_step"), (desc(elem=1), "input is"),
                   (desc(elem=3, qmax=0), "qmax"), (desc(elem=3, qmax=256), "qmax"), (desc(elem=3, scale=0.0), "scale"),
                   (desc(elem=3, scale=float("inf")), "scale"), (desc(elem=3, scale=float("nan")), "scale"),
                   (desc(h=4095, w=524417), "2^31"), (desc(elem=3, h=4095, w=2057), "2^31"), (desc(classes=17), "classes")):
        assert lib.oct_surf_workspace_bytes(C.byref(d)) == 0
        assert lib.oct_surf_extract(C.byref(d), order, None, None, None, None) == -22 and msg in L.last_error(), msg
    assert lib.oct_surf_workspace_bytes(C.byref(desc(elem=3, h=4095, w=2056))) > 0      # 255 * 4095 * 2056 < 2^31
    for bad, msg in (((0, 1, 1), "twice"), ((0, 1, 4), "classes 0..3"), ((0, -1, 2), "classes 0..3")):
        assert lib.oct_surf_extract(C.byref(desc()), (C.c_int32 * 3)(*bad), None, None, None, None) == -22 and msg in L.last_error()
    assert lib.oct_surf_extract(C.byref(desc()), None, None, None, None, None) == -22 and "null order" in L.last_error()
    assert lib.oct_surf_extract(C.byref(desc()), order, None, None, None, None) == -22 and "null input" in L.last_error()
    assert lib.oct_surf_extract(C.byref(desc(images=0)), order, None, None, None, None) == 0      # no image: a no-op
    keep = (C.c_int32 * 1)(2)
    assert lib.oct_surf_paint(C.byref(desc(nkeep=1)), order, keep, None, None, None, None) == -22 and "both keep and order" in L.last_error()
    assert lib.oct_surf_paint(C.byref(desc(nkeep=1)), order, None, None, None, None, None) == -22 and "null keep" in L.last_error()
    assert lib.oct_surf_error_update(C.byref(desc()), None, None, None, None, None) == -22 and "state" in L.last_error()
    assert lib.oct_surf_error_update(None, None, None, None, None, None) == -22 and "null descriptor" in L.last_error()
