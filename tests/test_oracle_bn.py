"""oracle/ref_bn.py (the float64 restatements that tests/test_gpu_bn.py holds csrc/bn.hip to) against torch's float64 CPU
operators and autograd.  No GPU.  In float64 the two agree to 1e-12 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_bn as B
from oracle.bounds import seed, stored

RTOL = 1e-12


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = RTOL * max(np.abs(ref).max(), 1.0)
    err = np.abs(got - ref).max()
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def nhwc(t):
    return t.detach().numpy().transpose(0, 2, 3, 1)


def stat_rows(y, nblocks=3):
    """partial rows [nblocks][2][c] as a convolution's epilogue leaves them: the pixels split into nblocks runs"""
    flat = y.reshape(-1, y.shape[-1])
    return np.stack([np.stack([p.sum(0), (p * p).sum(0)]) for p in np.array_split(flat, nblocks)])


def data(shape, tag):
    rng = np.random.default_rng(seed(shape, tag))
    n, h, w, c = shape
    y = stored(rng.standard_normal(shape) * 1.5 + 0.3, "bf16")      # few mantissa bits: no near-ties inside a window
    gamma = 1 + 0.3 * rng.standard_normal(c)
    beta = 0.2 * rng.standard_normal(c)
    da = rng.standard_normal(shape)
    dp = rng.standard_normal((n, h // 2, w // 2, c))
    return rng, y, gamma, beta, da, dp


SHAPES = [(3, 6, 10, 1), (2, 6, 10, 3), (1, 2, 2, 8), (3, 10, 14, 24), (2, 6, 6, 64)]
MODES = [(True, True), (True, False), (False, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("use_da,use_dp", MODES)
def test_chain_equals_autograd_of_batch_norm_relu_pool(shape, use_da, use_dp):
    """finalize -> relu (+ pool) -> reduce -> bwd_finalize -> apply == autograd of max_pool2d(relu(batch_norm(y))), with a second
    gradient entering at the un-pooled activation"""
    _, y, gamma, beta, da, dp = data(shape, "chain")
    n, h, w, c = shape
    eps = 1e-5
    x = nchw(y).requires_grad_(True)
    tg, tb = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    a = F.relu(F.batch_norm(x, None, None, tg, tb, training=True, eps=eps))
    p = F.max_pool2d(a, 2)
    loss = 0
    if use_da:
        loss = loss + (a * nchw(da)).sum()
    if use_dp:
        loss = loss + (p * nchw(dp)).sum()
    loss.backward()

    fin = B.bn_finalize(stat_rows(y), n * h * w, gamma, beta, eps)
    ra, _, _ = B.bn_relu(y, fin["scale"], fin["shift"])
    close(ra, nhwc(a), "relu(bn(y))")
    rp, _, _ = B.bn_relu_pool(y, fin["scale"], fin["shift"])
    close(rp, nhwc(p), "max_pool2d(relu(bn(y)))")
    red = B.dact_bn_reduce(da if use_da else None, dp if use_dp else None, y, fin["scale"], fin["shift"], fin["mean"], fin["invstd"])
    rows = np.stack([red["s1"], red["s2"]])[None]
    bf = B.bn_bwd_finalize(rows, n * h * w, gamma, fin["mean"], fin["invstd"])
    close(bf["dgamma"], tg.grad.numpy(), "dgamma")
    close(bf["dbeta"], tb.grad.numpy(), "dbeta")
    dy, _ = B.bn_bwd_apply(red["g"], y, bf["coef"])
    close(dy, nhwc(x.grad), "dy")
    # the mask re-derived in the apply (g = dA) and the pooled apply that never stores g
    if not use_dp:
        dy2, _ = B.bn_bwd_apply(da, y, bf["coef"], fin["scale"], fin["shift"])
        close(dy2, nhwc(x.grad), "dy, mask re-derived")
    else:
        dy3, _ = B.bn_bwd_apply_pool(da if use_da else None, dp, y, fin["scale"], fin["shift"], bf["coef"])
        close(dy3, nhwc(x.grad), "dy, pooled apply")


def test_bwd_finalize_accumulates():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((5, 2, 7))
    g, m, i = rng.standard_normal(7), rng.standard_normal(7), rng.uniform(0.5, 2, 7)
    d0, b0 = rng.standard_normal(7), rng.standard_normal(7)
    one = B.bn_bwd_finalize(rows, 11, g, m, i)
    acc = B.bn_bwd_finalize(rows, 11, g, m, i, d0, b0, accumulate=True)
    close(acc["dgamma"], d0 + one["dgamma"], "dgamma accumulate")
    close(acc["dbeta"], b0 + one["dbeta"], "dbeta accumulate")
    close(acc["coef"], one["coef"], "coef")


@pytest.mark.parametrize("plus_quarter", [False, True])
@pytest.mark.parametrize("use_da,use_dp", MODES)
def test_ties_route_and_mask_as_autograd(plus_quarter, use_da, use_dp):
    """integer-valued y: windows tie (first maximum in row-major order) and z == 0 occurs (relu'(0) = 0)"""
    shape = (2, 6, 10, 5)
    rng = np.random.default_rng(seed(shape, plus_quarter))
    y = rng.integers(-3, 4, shape).astype(np.float64)
    scale = np.array([0.5, -0.5, 1.0, -1.0, 2.0])
    shift = np.array([0.0, 0.5, -1.0, 1.0, 0.0]) + (0.25 if plus_quarter else 0.0)
    da = rng.integers(-2, 3, shape).astype(np.float64)
    dp = rng.integers(-2, 3, (2, 3, 5, 5)).astype(np.float64)
    z = (nchw(y) * torch.from_numpy(scale)[None, :, None, None] + torch.from_numpy(shift)[None, :, None, None]).requires_grad_(True)
    a = F.relu(z)
    loss = ((a * nchw(da)).sum() if use_da else 0) + ((F.max_pool2d(a, 2) * nchw(dp)).sum() if use_dp else 0)
    loss.backward()
    if not plus_quarter:
        assert (z == 0).any()
    win = nhwc(a).reshape(2, 3, 2, 5, 2, 5)
    assert (win[:, :, 0, :, 0] == win[:, :, 0, :, 1]).any(), "no tie inside a window"
    red = B.dact_bn_reduce(da if use_da else None, dp if use_dp else None, y, scale, shift, 0.0, 1.0)
    assert np.array_equal(red["g"], nhwc(z.grad))
    assert np.array_equal(red["s1"], nhwc(z.grad).sum((0, 1, 2)))


@pytest.mark.parametrize("shape", [(3, 7, 11, 1), (2, 7, 11, 8), (2, 5, 3, 24)], ids=lambda s: "x".join(map(str, s)))
def test_prelu_stages_equal_autograd(shape):
    rng, y, gamma, beta, da, _ = data(shape, "prelu")
    n, h, w, c = shape
    x = nchw(y).requires_grad_(True)
    tg, tb = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    act = torch.nn.PReLU().double()
    with torch.no_grad():
        act.weight.fill_(0.3)
    out = act(F.batch_norm(x, None, None, tg, tb, training=True, eps=1e-5))
    (out * nchw(da)).sum().backward()
    fin = B.bn_finalize(stat_rows(y, 2), n * h * w, gamma, beta, 1e-5)
    red = B.dact_bn_reduce_prelu(da, y, fin["scale"], fin["shift"], 0.3, fin["mean"], fin["invstd"])
    # z32 is z rounded to fp32: dalpha through it is within fp32 of autograd's, the rest is selection by sign
    zf = y * fin["scale"] + fin["shift"]
    close((np.where(zf > 0, 0.0, da * zf)).sum(), act.weight.grad.numpy()[0], "dalpha (float64 z)")
    assert abs(red["dalpha"] - act.weight.grad.numpy()[0]) <= 2.0 ** -23 * red["dalpha_terms"]
    bf = B.bn_bwd_finalize(np.stack([red["s1"], red["s2"]])[None], n * h * w, gamma, fin["mean"], fin["invstd"])
    close(bf["dgamma"], tg.grad.numpy(), "dgamma")
    close(bf["dbeta"], tb.grad.numpy(), "dbeta")
    dy, _ = B.bn_bwd_apply_prelu(da, y, bf["coef"], fin["scale"], fin["shift"], 0.3)
    close(dy, nhwc(x.grad), "dy")


def test_prelu_slope_branch_at_zero():
    shape = (2, 5, 7, 3)
    rng = np.random.default_rng(5)
    y = rng.integers(-2, 3, shape).astype(np.float64)
    scale, shift = np.array([1.0, -0.5, 2.0]), np.array([0.0, 0.5, -2.0])
    da = rng.integers(1, 5, shape).astype(np.float64)
    z = (nchw(y) * torch.from_numpy(scale)[None, :, None, None] + torch.from_numpy(shift)[None, :, None, None]).requires_grad_(True)
    act = torch.nn.PReLU().double()
    (act(z) * nchw(da)).sum().backward()
    assert (z == 0).any()
    dz, _ = B.prelu_dz(da, y, scale, shift, 0.25)
    assert np.array_equal(dz, nhwc(z.grad))
    assert (dz[nhwc(z) == 0] == 0.25 * da[nhwc(z) == 0]).all()
    red = B.dact_bn_reduce_prelu(da, y, scale, shift, 0.25, 0.0, 1.0)
    assert red["dalpha"] == act.weight.grad.numpy()[0]


@pytest.mark.parametrize("count_one", [False, True])
def test_running_statistics_with_a_conv_bias(count_one):
    shape = (1, 1, 1, 6) if count_one else (3, 5, 7, 6)
    rng, y, gamma, beta, _, _ = data(shape, "running")
    n, h, w, c = shape
    bias = rng.standard_normal(c)
    bn = torch.nn.BatchNorm2d(c, eps=1e-5, momentum=0.1).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
    rm, rv = np.zeros(c), np.ones(c)
    for step in range(2):
        ys = y * (1 + step)
        if count_one:   # torch refuses one value per channel in training mode: the running update is restated from its formula
            fin = B.bn_finalize(stat_rows(ys, 1), 1, gamma, beta, 1e-5, 0.1, bias, rm, rv)
            close(fin["running_mean"], 0.9 * rm + 0.1 * (ys.reshape(c) + bias), "running_mean, count 1")
            close(fin["running_var"], 0.9 * rv, "running_var, count 1 (variance 0, no n/(n-1))")
        else:
            out = bn(nchw(ys) + torch.from_numpy(bias)[None, :, None, None])
            fin = B.bn_finalize(stat_rows(ys, 4), n * h * w, gamma, beta, 1e-5, 0.1, bias, rm, rv)
            close(fin["running_mean"], bn.running_mean.numpy(), "running_mean")
            close(fin["running_var"], bn.running_var.numpy(), "running_var")
            close(ys * fin["scale"] + fin["shift"], nhwc(out), "the bias cancels in the train-mode output")
        rm, rv = fin["running_mean"], fin["running_var"]
    none = B.bn_finalize(stat_rows(y, 1), n * h * w, gamma, beta, 1e-5)
    assert none["running_mean"] is None and none["running_var"] is None


@pytest.mark.parametrize("with_bias", [False, True])
def test_eval_coeffs_equal_eval_mode_batch_norm(with_bias):
    shape = (2, 5, 7, 6)
    rng, y, gamma, beta, _, _ = data(shape, "eval")
    c = shape[-1]
    rm, rv = rng.standard_normal(c), rng.uniform(0.3, 2.0, c)
    bias = rng.standard_normal(c) if with_bias else None
    x = nchw(y) + (torch.from_numpy(bias)[None, :, None, None] if with_bias else 0)
    out = F.batch_norm(x, torch.from_numpy(rm), torch.from_numpy(rv), torch.from_numpy(gamma), torch.from_numpy(beta), training=False, eps=1e-5)
    scale, shift = B.bn_eval_coeffs(gamma, beta, rm, rv, 1e-5, bias)
    close(y * scale + shift, nhwc(out), "eval-mode batch_norm")


@pytest.mark.parametrize("fold", [1, 4])
def test_reduce_bias_partials(fold):
    rng = np.random.default_rng(fold)
    part = rng.standard_normal((5, fold * 6))
    ref = torch.from_numpy(part).view(5, fold, 6).sum((0, 1)).numpy()
    out, terms, count = B.reduce_bias_partials(part, 6)
    close(out, ref, "bias partials")
    assert count == 5 * fold and (terms >= np.abs(out)).all()
    old = rng.standard_normal(6)
    close(B.reduce_bias_partials(part, 6, old, accumulate=True)[0], ref + old, "bias partials, accumulate")


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("gscale", [1.0, 0.125])
def test_sgd_step_equals_torch_sgd(momentum, wd, gscale):
    rng = np.random.default_rng(seed(momentum, wd, gscale))
    p = rng.standard_normal(37)
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=0.05, momentum=momentum, weight_decay=wd)
    buf = np.zeros(37) if momentum else None
    for step in range(3):
        g = rng.standard_normal(37)
        tp.grad = torch.from_numpy(g * gscale)        # torch sees the gradient already multiplied by grad_scale
        opt.step()
        p, buf, _ = B.sgd_step(p, g, buf, 0.05, momentum, wd, gscale, first=step == 0)
        close(p, tp.detach().numpy(), f"parameters after step {step}")
        if momentum:
            close(buf, opt.state[tp]["momentum_buffer"].numpy(), f"momentum buffer after step {step}")
        else:
            assert buf is None
