"""oracle/ref_stream.py held to torch's CPU operators, so that a wrong restatement cannot hide a wrong kernel in
tests/test_gpu_streaming.py.  Small NHWC shapes with ties (integer-valued data), NaN and one-pixel axes; no GPU."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import ref_stream as R


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(a), -1, 1)))


def nhwc(t):
    return np.moveaxis(t.detach().numpy(), 1, -1)


BIL = [(1, 1, 1, 1), (1, 5, 1, 3), (5, 1, 3, 1), (3, 4, 6, 8), (7, 11, 14, 22), (9, 13, 4, 5), (6, 6, 6, 6), (31, 3, 62, 6),
       (62, 2, 124, 4), (2, 7, 1, 9)]


@pytest.mark.parametrize("h,w,ho,wo", BIL)
def test_bilinear_matches_torch_interpolate_and_its_autograd(h, w, ho, wo):
    rng = np.random.default_rng(h * 100 + ho)
    x = rng.standard_normal((2, h, w, 3))
    out, terms = R.bilinear_fwd(x, ho, wo)
    xt = nchw(x.astype(np.float32)).requires_grad_(True)
    ref = F.interpolate(xt, size=(ho, wo), mode="bilinear", align_corners=True)
    # torch evaluates in fp32 with the same fp32 source indices: agreement to fp32 rounding of the four-tap sum
    np.testing.assert_allclose(out, nhwc(ref), rtol=0, atol=4e-7 * terms.max() + 1e-12)
    assert np.all(terms >= np.abs(out) - 1e-12)
    d = rng.standard_normal((2, ho, wo, 3))
    ref.backward(nchw(d.astype(np.float32)))
    dx, dterms, count = R.bilinear_bwd(d, h, w)
    np.testing.assert_allclose(dx, nhwc(xt.grad), rtol=0, atol=1e-6 * max(1.0, dterms.max()))
    # the transpose property: <A x, d> == <x, A^T d>
    assert abs((out * d).sum() - (x * dx).sum()) < 1e-9 * max(1.0, np.abs(out * d).sum())
    assert count.max() >= 1


def test_bilinear_source_index_is_fp32():
    # (in-1)/(out-1) = 30/61 is not representable: the documented fp32 product picks the taps, as torch's fp32 kernel does
    i0, i1, lam = R.bilinear_taps(31, 62)
    r = np.float32(30) / np.float32(61)
    s = np.float32(r) * np.arange(62, dtype=np.float32)
    assert np.array_equal(i0, np.minimum(s.astype(np.int64), 30)) and i0[-1] == 30 and i1[-1] == 30
    assert np.all((lam >= 0) & (lam < 1))
    i0, i1, lam = R.bilinear_taps(1, 5)         # one-pixel input: every output reads pixel 0
    assert not i0.any() and not i1.any() and not lam.any()
    i0, _, lam = R.bilinear_taps(7, 1)          # one-pixel output: ratio 0, the first input pixel
    assert i0.tolist() == [0] and lam.tolist() == [0.0]


def _pool_input(rng, n, h, w, c, nan=True):
    a = rng.integers(-3, 4, (n, h, w, c)).astype(np.float32)     # few values: ties in most windows
    if nan:
        a[0, 0, 1, 0] = np.nan
        a[-1, h - 1, w - 1, c - 1] = np.nan
        if h > 2 and w > 2:
            a[0, 1, 0, 0] = np.nan                               # two NaN in one window
    return a


@pytest.mark.parametrize("n,h,w,c,k", [(2, 5, 7, 3, 2), (1, 6, 9, 8, 3), (2, 4, 4, 1, 2), (1, 2, 2, 5, 2), (1, 9, 5, 2, 4)])
def test_maxpool_matches_torch_with_ties_and_nan(n, h, w, c, k):
    rng = np.random.default_rng(h * w * c + k)
    a = _pool_input(rng, n, h, w, c)
    out, code = R.maxpool(a, k)
    at = nchw(a).requires_grad_(True)
    ref, idx = F.max_pool2d(at, k, k, return_indices=True)
    np.testing.assert_array_equal(out, nhwc(ref))                 # NaN propagates, like torch
    assert np.isnan(out).any()
    np.testing.assert_array_equal(R.maxpool_plane_index(code, k, w), nhwc(idx))
    d = rng.integers(1, 9, out.shape).astype(np.float32)
    ref.backward(nchw(d))
    np.testing.assert_array_equal(R.window_scatter(d, code, k, h, w), nhwc(at.grad))
    # MaxUnpool2d forward = index scatter; its backward = index gather
    # (the plane is the input's, trailing rows / columns of the floor mode included)
    up = nn.MaxUnpool2d(k, k)(nchw(d), idx, output_size=(h, w))
    np.testing.assert_array_equal(R.index_scatter(d, nhwc(idx), h, w), nhwc(up))
    np.testing.assert_array_equal(R.index_scatter(d, nhwc(idx), h, w), R.window_scatter(d, code, k, h, w))
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    np.testing.assert_array_equal(R.index_gather(x, nhwc(idx)), R.window_gather(x, code, k))
    np.testing.assert_array_equal(R.index_gather(x, nhwc(idx)), nhwc(torch.gather(nchw(x).flatten(2), 2, idx.flatten(2)).view(idx.shape)))


def test_maxpool_first_maximum_wins_ties():
    a = np.ones((1, 4, 4, 2), np.float32)
    out, code = R.maxpool(a, 2)
    assert not code.any() and np.array_equal(out, np.ones((1, 2, 2, 2), np.float32))
    _, idx = F.max_pool2d(nchw(a), 2, 2, return_indices=True)
    assert np.array_equal(R.maxpool_plane_index(code, 2, 4), nhwc(idx))


@pytest.mark.parametrize("s,cout", [(2, 3), (4, 2), (1, 5), (3, 1)])
def test_depth_to_space_is_pixel_shuffle_after_the_channel_permutation(s, cout):
    rng = np.random.default_rng(s * 10 + cout)
    x = rng.standard_normal((2, 3, 5, s * s * cout)).astype(np.float32)
    # kernel channel order (dy*s+dx)*cout + co -> torch's co*s*s + dy*s + dx
    xt = x.reshape(2, 3, 5, s * s, cout).transpose(0, 1, 2, 4, 3).reshape(2, 3, 5, s * s * cout)
    ref = nhwc(F.pixel_shuffle(nchw(xt), s))
    np.testing.assert_array_equal(R.depth_to_space(x, s), ref)
    np.testing.assert_array_equal(R.space_to_depth(ref, s), x)
    np.testing.assert_array_equal(nhwc(F.pixel_unshuffle(nchw(ref), s)), xt)
    b = rng.standard_normal(cout)
    np.testing.assert_array_equal(R.depth_to_space(x, s, b), ref.astype(np.float64) + b)


@pytest.mark.parametrize("alpha", [0.25, -0.5, 0.0])
def test_prelu_matches_torch_and_its_autograd(alpha):
    rng = np.random.default_rng(7)
    y = rng.integers(-4, 5, (2, 5, 7, 3)).astype(np.float64)      # z == 0 occurs
    sc, sh = np.array([1.0, -0.5, 2.0]), np.array([0.0, 0.5, -1.0])
    out, terms, z = R.affine_prelu(y, sc, sh, alpha)
    assert (z == 0).any()
    zt = nchw(z).requires_grad_(True)
    wt = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
    ref = F.prelu(zt, wt)
    np.testing.assert_array_equal(out, nhwc(ref))
    d = rng.standard_normal(out.shape)
    ref.backward(nchw(d))
    dz, dalpha, aterms = R.affine_prelu_bwd(d, z, alpha)
    np.testing.assert_allclose(dz, nhwc(zt.grad), rtol=1e-15, atol=0)
    np.testing.assert_allclose(dalpha, float(wt.grad), rtol=1e-12, atol=1e-12)
    assert aterms >= abs(dalpha)


def test_depth_pool_matches_maxpool3d_with_ties_and_nan():
    rng = np.random.default_rng(3)
    vol = rng.integers(-2, 3, (2, 4, 6, 5, 3)).astype(np.float32)    # N D H W C: ties between the two slices
    vol[0, 1, 2, 3, 1] = np.nan
    vol[1, 2, 0, 0, 0] = np.nan
    vol[1, 3, 0, 0, 0] = np.nan
    n, d, h, w, c = vol.shape
    p2 = vol.reshape(n * d // 2, 2, h * w * c)
    out, _ = R.depth_pool(p2)
    vt = torch.from_numpy(np.ascontiguousarray(vol.transpose(0, 4, 1, 2, 3))).requires_grad_(True)
    ref, idx = F.max_pool3d(vt, (2, 1, 1), (2, 1, 1), return_indices=True)
    refn = ref.detach().numpy().transpose(0, 2, 3, 4, 1).reshape(n * d // 2, h * w * c)
    np.testing.assert_array_equal(out, refn)
    g = rng.integers(1, 5, refn.shape).astype(np.float32)
    ref.backward(torch.from_numpy(np.ascontiguousarray(g.reshape(n, d // 2, h, w, c).transpose(0, 4, 1, 2, 3))))
    grad = vt.grad.numpy().transpose(0, 2, 3, 4, 1).reshape(n * d // 2, 2, h * w * c)
    np.testing.assert_array_equal(R.depth_pool_bwd(p2, g), grad)


def test_affine_act_and_act_bwd_match_torch():
    rng = np.random.default_rng(5)
    y, res = rng.standard_normal((2, 3, 5, 4)), rng.standard_normal((2, 3, 5, 4))
    sc, sh, rb = rng.standard_normal(4), rng.standard_normal(4), rng.standard_normal(4)
    store = lambda v: torch.from_numpy(v).to(torch.bfloat16).double().numpy()  # noqa: E731
    for act, fn in ((R.ACT_NONE, lambda t: t), (R.ACT_RELU, torch.relu), (R.ACT_SIGMOID, torch.sigmoid)):
        out, terms, z = R.affine_act(y, sc, sh, act, res, rb, store)
        zt = torch.from_numpy(y * sc + sh + store(res + rb)).requires_grad_(True)
        ref = fn(zt)
        np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-15, atol=1e-15)
        assert np.all(terms >= np.abs(z) - 1e-12)
        if act != R.ACT_NONE:
            d = rng.standard_normal(out.shape)
            ref.backward(torch.from_numpy(d))
            np.testing.assert_allclose(R.act_bwd(d, out, act), zt.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_gate_rowdot_channel_sum_match_torch():
    rng = np.random.default_rng(9)
    x, p, d = rng.standard_normal((2, 3, 5, 6)), rng.random((2, 3, 5, 1)), rng.standard_normal((2, 3, 5, 6))
    xt, pt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(p).requires_grad_(True)
    (xt * pt).backward(torch.from_numpy(d))
    np.testing.assert_allclose(R.gate_fwd(x, p), x * p)
    dx, dp, _ = R.gate_bwd(d, x, p)
    np.testing.assert_allclose(dx, xt.grad.numpy(), rtol=1e-15)
    np.testing.assert_allclose(dp, pt.grad.numpy(), rtol=1e-12)
    xr, dy = rng.standard_normal((37, 16)), rng.standard_normal((37, 5))
    wt, bt = torch.zeros(5, 16, dtype=torch.float64, requires_grad=True), torch.zeros(5, dtype=torch.float64, requires_grad=True)
    F.linear(torch.from_numpy(xr), wt, bt).backward(torch.from_numpy(dy))
    dw, db, _, _ = R.rowdot_bwd_weight(dy, xr)
    np.testing.assert_allclose(dw, wt.grad.numpy(), rtol=1e-12)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-12)
    s, _ = R.channel_sum(x)
    np.testing.assert_allclose(s, torch.from_numpy(x).sum((0, 1, 2)).numpy(), rtol=1e-12)
