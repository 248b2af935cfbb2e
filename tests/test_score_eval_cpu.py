"""CPU: the key of the score evaluator and `evaluation.score_metrics_from_state` on states made by the numpy restatement
tests/score_ref.py -- no GPU, no kernel.  sklearn is the reference for AUC / average precision only (importorskip inside those
tests); every comparison of counts is on integers and exact, the float formulas are compared with == against Metrics._formulas
on the same counts."""
import numpy as np
import pytest

import score_ref as R
from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation as E
from retinal_oct_image_segmentation_via_deep_learning_amd.Metrics import _formulas

GRID = np.array(R.GRID, dtype=np.float32)


def _sample():
    rng = np.random.default_rng(11)
    v = np.concatenate([(3.0 * rng.standard_normal(20000)).astype(np.float32),
                        rng.integers(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        R.special_values()])
    return np.sort(v[~np.isnan(v)])


# ---- the key ----------------------------------------------------------------------------------------------------------------
def test_key16_is_the_restatements_key():
    v = _sample()
    np.testing.assert_array_equal(E.key16(v), R.key16(v))
    assert E.SCORE_KEYS == R.KEYS and E.score_state_size(3) == R.state_size(3) == 3 * (2 * 65536 + 3) + 1


def test_key16_is_monotone_and_stays_in_range():
    v = _sample()
    k = E.key16(v)
    assert (np.diff(k) >= 0).all()
    assert k.min() >= 0x0080 and k.max() <= 0xFF80


def test_key16_special_values():
    fi = np.finfo(np.float32)
    f = np.float32
    assert E.key16(f(0.0)) == E.key16(f(-0.0)) == 0x8000
    assert E.key16(f(np.inf)) == 0xFF80 and E.key16(f(-np.inf)) == 0x0080
    assert E.key16(fi.max) == 0xFF7F
    assert E.key16(-fi.max) == 0x0080          # not on the bf16 grid: rounded toward -inf it shares the bin of -inf
    assert E.key16(np.float32(-3.3895314e38)) == 0x0081   # the largest finite bf16 magnitude, negated, is its own bin
    # the smallest positive denormal sits in the bin of +0, its negative rounds down to the first negative bin
    assert E.key16(fi.smallest_subnormal) == 0x8000 and E.key16(-fi.smallest_subnormal) == 0x7FFF
    # bf16 has denormals too: 2^-127 is a grid point on both sides
    assert E.key16(f(fi.tiny / 2)) == 0x8040 and E.key16(f(-fi.tiny / 2)) == 0x8000 - 0x0040
    # the smallest normals are on the grid
    assert E.key16(fi.tiny) == 0x8080 and E.key16(-fi.tiny) == 0x8000 - 0x0080
    assert E.key_value(0x8000) == 0.0 and np.isinf(E.key_value(0xFF80)) and np.isinf(E.key_value(0x0080))


def test_grid_thresholds_split_every_float_exactly():
    v = np.concatenate([_sample(), R.ulp_neighbours(GRID)])
    k = E.key16(v)
    for g in GRID:
        kg = E.key16(g)
        assert E.key_value(kg) == g, g
        np.testing.assert_array_equal(v >= g, k >= kg, err_msg=str(g))
        below, above = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert E.key16(below) == kg - 1 and E.key16(above) == kg, g          # [g(k), g(k+1)): half-open


# ---- score_metrics_from_state -------------------------------------------------------------------------------------------
def _case(kind, channels=2):
    rng = np.random.default_rng(R.KEYS + channels)
    t, s = R.random_field(rng, (2, channels, 24, 40))                          # 1920 elements per channel
    if kind == "bf16":
        s = R.to_bf16_values(s)
    return t, s, R.score_state(t, s, channels)


def test_bf16_scores_give_sklearns_auc_and_average_precision():
    sk = pytest.importorskip("sklearn.metrics")
    t, s, st = _case("bf16")
    m = E.score_metrics_from_state(st, 2)
    for c in range(2):
        tc, sc = t[:, c].ravel(), s[:, c].ravel()
        auc, ap = sk.roc_auc_score(tc, sc), sk.average_precision_score(tc, sc)
        assert abs(m["auc"][c] - auc) <= 1e-12
        assert abs(m["average_precision"][c] - ap) <= 1e-12
        assert m["auc_lo"][c] <= m["auc"][c] <= m["auc_hi"][c]


def test_uint8_scores_give_sklearns_auc():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    s8 = rng.integers(0, 256, size=(1, 1, 30, 64)).astype(np.uint8)
    t = (s8.astype(np.float32) + 60.0 * rng.standard_normal(s8.shape) > 128).astype(np.uint8)
    m = E.score_metrics_from_state(R.score_state(t, s8.astype(np.float32), 1), 1, logits=False)
    assert abs(m["auc"][0] - sk.roc_auc_score(t.ravel(), s8.ravel())) <= 1e-12
    assert abs(m["average_precision"][0] - sk.average_precision_score(t.ravel(), s8.ravel())) <= 1e-12


def test_fp32_scores_bracket_sklearns_auc():
    sk = pytest.importorskip("sklearn.metrics")
    t, s, st = _case("fp32")
    m = E.score_metrics_from_state(st, 2)
    for c in range(2):
        exact = sk.roc_auc_score(t[:, c].ravel(), s[:, c].ravel())
        assert m["auc_lo"][c] <= exact <= m["auc_hi"][c]
        assert 0 < m["auc_hi"][c] - m["auc_lo"][c] < 0.01


@pytest.mark.parametrize("kind", ["bf16", "fp32"])
def test_counts_at_one_half_are_the_counts_of_scores_ge_zero_and_the_formulas_are_formulas(kind):
    t, s, st = _case(kind)
    m = E.score_metrics_from_state(st, 2, thresholds=(0.5, 0.3, 0.9))
    assert m["counts"].shape == (2, 3, 6) and m["counts"].dtype == np.int64
    assert m["threshold_used"].dtype == np.float32 and m["threshold_used"][0] == 0.0
    for c in range(2):
        tc, pc = t[:, c].ravel() == 1, s[:, c].ravel() >= 0
        want = [(tc & pc).sum(), tc.sum(), pc.sum(), (~tc & ~pc).sum(), (~tc & pc).sum(), (tc & ~pc).sum()]
        np.testing.assert_array_equal(m["counts"][c, 0], want)
        assert m["positives"][c] == tc.sum() and m["negatives"][c] == (~tc).sum()
        for i in range(3):
            # any threshold: the counts of score >= threshold_used
            pi = s[:, c].ravel() >= m["threshold_used"][i]
            np.testing.assert_array_equal(m["counts"][c, i], [(tc & pi).sum(), tc.sum(), pi.sum(), (~tc & ~pi).sum(),
                                                              (~tc & pi).sum(), (tc & ~pi).sum()])
            f = _formulas(*(int(v) for v in m["counts"][c, i]), tc.size)
            for k, v in f.items():
                assert m[k].shape == (2, 3) and m[k][c, i] == v, k
    # the threshold actually used is the lower edge of the bin of mask_threshold(tau)
    from retinal_oct_image_segmentation_via_deep_learning_amd.losses import mask_threshold
    for i, tau in enumerate((0.5, 0.3, 0.9)):
        theta = np.float32(mask_threshold(tau))
        assert m["threshold_used"][i] <= theta and m["threshold_used"][i] == E.key_value(R.key16(theta))
    # probabilities instead of logits: the threshold is float32(tau) itself
    mp = E.score_metrics_from_state(st, 2, thresholds=(0.5,), logits=False)
    assert mp["threshold_used"][0] == np.float32(0.5)


def test_best_dice_is_the_brute_force_maximum_and_its_largest_threshold():
    t, s, st = _case("bf16")
    m = E.score_metrics_from_state(st, 2)
    for c in range(2):
        tc, sc = t[:, c].ravel() == 1, s[:, c].ravel()
        best, thr = -1.0, None
        for k in np.unique(R.key16(sc))[::-1]:                                # descending: the first maximum is the largest
            theta = E.key_value(k)
            p = sc >= theta
            d = _formulas(int((tc & p).sum()), int(tc.sum()), int(p.sum()), int((~tc & ~p).sum()), int((~tc & p).sum()),
                          int((tc & ~p).sum()), tc.size)["dice_coefficient"]
            if d > best:
                best, thr = d, theta
        assert m["best_dice"][c] == best and m["best_dice_threshold"][c] == thr


def test_curves_are_the_cumulative_counts_over_the_occupied_keys():
    t, s, st = _case("bf16")
    r = E.score_curves_from_state(st, 2, 1)
    tc, sc = t[:, 1].ravel() == 1, s[:, 1].ravel()
    assert (np.diff(r["thresholds"]) < 0).all() and r["thresholds"].size == np.unique(R.key16(sc)).size
    for i in (0, r["thresholds"].size // 2, r["thresholds"].size - 1):
        p = sc >= r["thresholds"][i]
        assert r["tp"][i] == (tc & p).sum() and r["fp"][i] == (~tc & p).sum()
    assert r["tpr"][-1] == 1.0 and r["fpr"][-1] == 1.0
    sk = pytest.importorskip("sklearn.metrics")
    fpr, tpr, _ = sk.roc_curve(tc, sc, drop_intermediate=False)
    np.testing.assert_array_equal(fpr[1:], r["fpr"])
    np.testing.assert_array_equal(tpr[1:], r["tpr"])


def test_a_missing_label_gives_nan_and_no_exception():
    t, s = R.constant_field((1, 2, 5, 7), value=-3.0, label=0)
    t[:, 1] = 1
    m = E.score_metrics_from_state(R.score_state(t, s, 2), 2)
    assert np.isnan(m["auc"]).all() and np.isnan(m["auc_lo"]).all() and np.isnan(m["auc_hi"]).all()
    assert np.isnan(m["average_precision"][0]) and m["average_precision"][1] == 1.0
    np.testing.assert_array_equal(m["counts"][:, 0], [[0, 0, 0, 35, 0, 0], [0, 35, 0, 0, 0, 35]])
    empty = E.score_metrics_from_state(np.zeros(R.state_size(1), dtype=np.int64), 1)
    assert np.isnan(empty["auc"][0]) and np.isnan(empty["best_dice"][0]) and empty["updates"] == 0


def test_counts_near_two_to_the_forty_per_bin_do_not_overflow():
    big = 2 ** 40
    st = np.zeros(R.state_size(1), dtype=np.int64)
    hist = st[:2 * R.KEYS].reshape(2, R.KEYS)
    k = R.key16(np.array([-1.0, 0.0, 1.0], dtype=np.float32))
    hist[0, k] = [3 * big, 2 * big, big]          # negatives mostly low
    hist[1, k] = [big, 2 * big, 3 * big]          # positives mostly high
    m = E.score_metrics_from_state(st, 1)
    # P = N = 6 * 2^40, P * N = 36 * 2^80 > 2^63.  wins = 2*3 + 3*(3+2) = 21, ties = 3 + 4 + 3 = 10 (in units of 2^80)
    assert m["positives"][0] == m["negatives"][0] == 6 * big
    assert m["auc"][0] == (21 + 5) / 36 and m["auc_lo"][0] == 21 / 36 and m["auc_hi"][0] == 31 / 36
    # descending: precision 3/4, 5/8, 6/12 with recall steps 3/6, 2/6, 1/6
    assert abs(m["average_precision"][0] - (3 / 6 * 3 / 4 + 2 / 6 * 5 / 8 + 1 / 6 * 6 / 12)) <= 1e-15
    np.testing.assert_array_equal(m["counts"][0, 0], [5 * big, 6 * big, 8 * big, 3 * big, 3 * big, big])


def test_state_and_argument_checks():
    with pytest.raises(ValueError):
        E.score_metrics_from_state(np.zeros(5, dtype=np.int64), 1)
    with pytest.raises(ValueError):
        E.score_metrics_from_state(np.zeros(R.state_size(1), dtype=np.float64), 1)
    with pytest.raises(ValueError):
        E.score_metrics_from_state(np.zeros(R.state_size(1), dtype=np.int64), 1, thresholds=(1.5,))
    with pytest.raises(ValueError):
        E.ScoreEvaluator(0)
    with pytest.raises(ValueError):
        E.ScoreEvaluator(2, ignore_value=1)
    with pytest.raises(TypeError):
        E.ScoreEvaluator(2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ScoreEvaluator(1, device="cpu")


def test_restatement_routes_every_element_to_one_place():
    rng = np.random.default_rng(2)
    t, s = R.special_field(rng, (2, 3, 5, 7))
    t[rng.random(t.shape) < 0.25] = 255
    t[rng.random(t.shape) < 0.1] = 2
    for ign in (None, 255):
        st = R.score_state(t, s, 3, ign)
        assert st[:-1].sum() == t.size and st[-1] == 1
        m = E.score_metrics_from_state(st, 3)
        assert (m["ignored"] == ((t == 255).sum(axis=(0, 2, 3)) if ign else 0)).all()
        assert (m["invalid"] == ((t > 1) & (t != (ign or -1))).sum(axis=(0, 2, 3))).all()
        assert m["nan"].sum() > 0
