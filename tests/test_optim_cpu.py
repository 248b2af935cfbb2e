"""CPU: the float64 restatements of tests/optim_ref.py against torch, the host logic of optim.FlatParams (split / join, the
weight-decay mask), the torch-compatible state-dict layout, and the host-side refusals of the optimizer exports."""
import copy
import inspect

import numpy as np
import pytest
import torch

import optim_ref as R
from oracle.bounds import seed


@pytest.fixture(scope="module")
def L():
    import os
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    _lib.lib()
    return _lib


def small_unet():
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    torch.manual_seed(3)
    return UNet(1, 4, init_features=8, compute_dtype="f32")


# ------------------------------------------------------------------------------------------------------------------
# 1. restatements against torch in float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_restatement_equals_torch_in_float64(decoupled, wd):
    rng = np.random.default_rng(seed("adam-ref", decoupled, wd))
    n, lr, b1, b2, eps = 301, 3e-3, 0.9, 0.999, 1e-8
    p = rng.standard_normal(n)
    ref = torch.from_numpy(p.copy()).requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    topt = cls([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 6):                                         # t = 1 included
        g = rng.standard_normal(n)
        ref.grad = torch.from_numpy(g.copy())
        topt.step()
        p, m, v, _ = R.adam_step(p, g, m, v, R.scalars(lr, b1, b2, eps, wd, t, fp32=False), decoupled)
        st = topt.state[ref]
        for got, want, what in ((p, ref.detach().numpy(), "p"), (m, st["exp_avg"].numpy(), "m"), (v, st["exp_avg_sq"].numpy(), "v")):
            assert np.abs(got - want).max() <= 1e-12, (what, t, np.abs(got - want).max())
    assert float(st["step"]) == 5


@pytest.mark.parametrize("max_norm", [0.5, 1e3])                  # the norm is about 17: above and below max_norm
def test_clip_restatement_equals_clip_grad_norm(max_norm):
    rng = np.random.default_rng(11)
    parts = [rng.standard_normal(s) for s in ((7, 3), (40,), (2, 5, 5), (193,))]
    params = [torch.zeros(a.shape, dtype=torch.float64, requires_grad=True) for a in parts]
    for q, a in zip(params, parts):
        q.grad = torch.from_numpy(a.copy())
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    flat = np.concatenate([a.reshape(-1) for a in parts])
    norm, coef = R.clip(flat, 1.0, max_norm)
    assert abs(norm - float(total)) <= 1e-12 * norm
    assert (coef < 1.0) == (norm > max_norm)
    got = np.concatenate([q.grad.numpy().reshape(-1) for q in params])
    assert np.abs(got - flat * coef).max() <= 1e-12
    # grad_scale multiplies the gradient before the norm
    norm2, _ = R.clip(flat, 0.25, max_norm)
    assert abs(norm2 - 0.25 * norm) <= 1e-12 * norm
    # non-finite gradients: torch's error_if_nonfinite=False behaviour
    bad = flat.copy()
    bad[5] = np.nan
    n3, c3 = R.clip(bad, 1.0, max_norm)
    assert np.isnan(n3) and np.isnan(c3)
    bad[5] = np.inf
    n4, c4 = R.clip(bad, 1.0, max_norm)
    assert np.isinf(n4) and c4 == 0.0


def test_torch_fp32_recurrence_deviates_from_float64():
    """the yardstick of the GPU recurrence test: torch's own fp32 AdamW against its float64 AdamW, 50 steps"""
    n = sum(p.numel() for p in small_unet().parameters())
    p0, grads = R.recurrence_inputs(n)
    d = np.abs(R.torch_adamw_recurrence(p0, grads, torch.float32) - R.torch_adamw_recurrence(p0, grads, torch.float64)).max()
    print(f"torch fp32 AdamW vs float64 after {R.REC_STEPS} steps, n = {n}: max deviation {d:.3e}")
    assert np.isfinite(d) and d > 0


# ------------------------------------------------------------------------------------------------------------------
# 2. FlatParams: split / join, decay mask
# ------------------------------------------------------------------------------------------------------------------
def test_flat_params_split_join_and_decay_mask():
    from retinal_oct_image_segmentation_via_deep_learning_amd.optim import _ALIGN, NO_DECAY_1D, FlatParams
    assert _ALIGN == R.CHUNK
    model = small_unet()
    lay = FlatParams(list(model.named_parameters()))
    numels = [p.numel() for p in lay.params]
    pad = np.ones(lay.total, bool)
    for o, k in zip(lay.offsets, numels):
        pad[o:o + k] = False
    assert pad.any(), "no alignment padding in this model"
    # no chunk is shared by two parameters
    ends = lay.offsets[1:] + [lay.total]
    assert all(o % _ALIGN == 0 for o in lay.offsets) and lay.total % _ALIGN == 0
    assert all(o + k <= e for o, k, e in zip(lay.offsets, numels, ends))
    owner = np.full(lay.total // _ALIGN, -1)
    for i, (o, k) in enumerate(zip(lay.offsets, numels)):
        c = slice(o // _ALIGN, (o + k + _ALIGN - 1) // _ALIGN)
        assert (owner[c] == -1).all(), f"{lay.names[i]} shares a chunk"
        owner[c] = i
    assert (owner >= 0).all()

    # split / join round trip, padding written as zero
    gen = torch.Generator().manual_seed(5)
    flat = torch.randn(lay.total, generator=gen)
    parts = lay.split(flat)
    assert [tuple(t.shape) for t in parts] == [tuple(p.shape) for p in lay.params]
    assert all(t.data_ptr() != flat.data_ptr() for t in parts), "split returns copies"
    back = lay.join(parts)
    want = flat.clone()
    want[torch.from_numpy(pad)] = 0
    assert torch.equal(back, want)
    out = torch.full((lay.total,), float("nan"))
    assert lay.join(parts, out=out) is out and torch.equal(out, want)
    assert torch.equal(torch.cat([t.reshape(-1) for t in lay.split(back)]), torch.cat([t.reshape(-1) for t in parts]))
    with pytest.raises(ValueError):
        lay.join(parts[:-1])
    wrong = list(parts)
    wrong[0] = wrong[0].reshape(-1)[:-1]
    with pytest.raises(ValueError):
        lay.join(wrong)
    with pytest.raises(ValueError):
        lay.split(flat[:-1])

    # the mask: BatchNorm parameters and biases 0, convolution weights 1
    mask = lay.decay_mask(NO_DECAY_1D)
    assert mask.dtype == torch.uint8 and mask.device.type == "cpu" and mask.numel() == lay.total // _ALIGN
    excluded = [p.ndim <= 1 for p in lay.params]
    assert any(excluded) and not all(excluded)
    assert np.array_equal(mask.numpy(), R.chunk_mask(lay.offsets, numels, lay.total, excluded))
    for name, p in zip(lay.names, lay.params):
        lo, hi = lay.span(name)
        m = mask[lo // _ALIGN:hi // _ALIGN]
        if "norm" in name or name.endswith(".bias"):
            assert p.ndim == 1 and not m.any(), name
        else:
            assert p.ndim == 4 and bool(m.all()), name
    assert bool(lay.decay_mask(None).all())
    assert not lay.decay_mask(lambda n, p: True).any()


# ------------------------------------------------------------------------------------------------------------------
# 3. state-dict layout, through the FlatParams helpers on CPU buffers
# ------------------------------------------------------------------------------------------------------------------
def _cpu_optimizer(cls, **kw):
    """A FusedSGD / FusedAdam whose buffers live on the CPU: everything but step() is host logic.  The constructor refuses CPU
    parameters, so the object is assembled from the layout as the constructor would."""
    from retinal_oct_image_segmentation_via_deep_learning_amd import optim as O
    model = small_unet()
    opt = cls.__new__(cls)
    opt.layout = O.FlatParams(list(model.named_parameters()))
    opt.params, opt.flat_p, opt.flat_g = opt.layout.params, opt.layout.flat_p, opt.layout.flat_g
    opt.steps, opt.max_grad_norm, opt.last_grad_norm, opt.no_decay, opt.decay_mask = 0, None, None, None, None
    for k, v in kw.items():
        setattr(opt, k, v)
    return model, opt


def test_adam_state_dict_loads_into_torch_and_back():
    from retinal_oct_image_segmentation_via_deep_learning_amd import optim as O
    model, opt = _cpu_optimizer(O.FusedAdam, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.0, decoupled=False)
    gen = torch.Generator().manual_seed(9)
    opt.exp_avg = opt.layout.join([torch.randn(p.shape, generator=gen) for p in opt.params])
    opt.exp_avg_sq = opt.layout.join([torch.rand(p.shape, generator=gen) for p in opt.params])
    assert opt.state_dict()["state"] == {}, "no state before the first step"
    opt.steps = 7
    sd = opt.state_dict()
    n = len(opt.params)
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == list(range(n))
    assert len(sd["param_groups"]) == 1 and sd["param_groups"][0]["params"] == list(range(n))
    for i, p in enumerate(opt.params):
        s = sd["state"][i]
        assert sorted(s) == ["exp_avg", "exp_avg_sq", "step"]
        assert s["step"].dtype == torch.float32 and float(s["step"]) == 7.0
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape
    # into torch.optim.Adam over CPU copies of the same parameters
    copies = [p.detach().clone().requires_grad_(True) for p in opt.params]
    topt = torch.optim.Adam(copies, foreach=False)
    topt.load_state_dict(sd)
    g = topt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.99), 1e-7, 0.0)
    for i, c in enumerate(copies):
        assert torch.equal(topt.state[c]["exp_avg"], sd["state"][i]["exp_avg"]) and float(topt.state[c]["step"]) == 7.0
    for c in copies:                                              # torch can step from it
        c.grad = torch.ones_like(c)
    topt.step()
    # and torch's dict loads back
    tsd = topt.state_dict()
    _, other = _cpu_optimizer(O.FusedAdam, lr=0.0, betas=(0.0, 0.0), eps=1.0, weight_decay=1.0, decoupled=True)
    other.exp_avg, other.exp_avg_sq = torch.zeros_like(other.flat_p), torch.zeros_like(other.flat_p)
    other.load_state_dict(tsd)
    assert other.steps == 8 and (other.lr, other.betas, other.eps, other.weight_decay, other.decoupled) == \
        (2e-3, (0.8, 0.99), 1e-7, 0.0, False)
    assert torch.equal(other.exp_avg, other.layout.join([topt.state[c]["exp_avg"] for c in copies]))
    assert torch.equal(other.exp_avg_sq, other.layout.join([topt.state[c]["exp_avg_sq"] for c in copies]))
    pad = torch.ones(other.layout.total, dtype=torch.bool)
    for p, o in zip(other.params, other.layout.offsets):
        pad[o:o + p.numel()] = False
    assert not other.exp_avg[pad].any() and not other.exp_avg_sq[pad].any()
    # mismatches
    short = copy.deepcopy(tsd)
    short["param_groups"][0]["params"] = short["param_groups"][0]["params"][:-1]
    with pytest.raises(ValueError):
        other.load_state_dict(short)
    bent = copy.deepcopy(tsd)
    bent["state"][0]["exp_avg"] = bent["state"][0]["exp_avg"].reshape(-1)
    with pytest.raises(ValueError):
        other.load_state_dict(bent)


def test_sgd_state_dict_loads_into_torch_and_back():
    from retinal_oct_image_segmentation_via_deep_learning_amd import optim as O
    model, opt = _cpu_optimizer(O.FusedSGD, lr=0.05, momentum=0.9, weight_decay=1e-3)
    gen = torch.Generator().manual_seed(10)
    opt.buf = opt.layout.join([torch.randn(p.shape, generator=gen) for p in opt.params])
    assert opt.state_dict()["state"] == {}, "momentum_buffer is absent before the first step"
    opt.steps = 3
    sd = opt.state_dict()
    n = len(opt.params)
    assert all(sorted(sd["state"][i]) == ["momentum_buffer"] and sd["state"][i]["momentum_buffer"].shape == p.shape
               for i, p in enumerate(opt.params))
    copies = [p.detach().clone().requires_grad_(True) for p in opt.params]
    topt = torch.optim.SGD(copies, lr=1.0, momentum=0.1, foreach=False)
    topt.load_state_dict(sd)
    g = topt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (0.05, 0.9, 1e-3, False)
    for c in copies:
        c.grad = torch.ones_like(c)
    topt.step()
    tsd = topt.state_dict()
    tsd["param_groups"][0].pop("steps", None)                     # a dict that torch itself wrote has no such key
    _, other = _cpu_optimizer(O.FusedSGD, lr=0.0, momentum=0.0, weight_decay=0.0, buf=None)
    other.load_state_dict(tsd)
    assert (other.lr, other.momentum, other.weight_decay) == (0.05, 0.9, 1e-3)
    assert other.steps >= 1, "a loaded momentum buffer clears the first-step flag"
    assert torch.equal(other.buf, other.layout.join([topt.state[c]["momentum_buffer"] for c in copies]))
    other.load_state_dict(sd)
    assert other.steps == 3
    # a dict from before the first step restores the first-step flag
    fresh = torch.optim.SGD(copies, lr=0.05, momentum=0.9).state_dict()
    other.load_state_dict(fresh)
    assert other.steps == 0 and not other.buf.any()
    short = copy.deepcopy(sd)
    del short["state"][n - 1]
    with pytest.raises(ValueError):
        other.load_state_dict(short)


# ------------------------------------------------------------------------------------------------------------------
# 4. host-side refusals
# ------------------------------------------------------------------------------------------------------------------
def test_optimizer_exports_refuse_bad_arguments_without_a_gpu(L):
    lib = L.lib()
    x = 4096                                                      # never dereferenced: every call below is refused before a launch

    def refused(rc):
        assert rc == -22, rc
        assert L.last_error()

    adam = lambda *a: lib.oct_adam_step(*a)                       # noqa: E731
    ok = [x, x, x, x, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1e-2, 31.6, 1.0, None, None, None]

    def but(i, val):
        a = list(ok)
        a[i] = val
        return a
    for i in range(4):
        refused(adam(*but(i, None)))
    refused(adam(*but(4, 0)))
    assert "n == 0" in L.last_error()
    refused(adam(*but(8, 0.0)))
    assert "eps" in L.last_error()
    refused(adam(*but(8, -1e-8)))
    for i in (6, 7):
        refused(adam(*but(i, 1.0)))
        assert "betas" in L.last_error()
        refused(adam(*but(i, -0.1)))
    refused(adam(*but(11, float("nan"))))
    refused(adam(*but(12, 0.5)))

    refused(lib.oct_grad_norm(None, 16, 1.0, 1.0, x, x, None))
    refused(lib.oct_grad_norm(x, 16, 1.0, 1.0, None, x, None))
    refused(lib.oct_grad_norm(x, 16, 1.0, 1.0, x, None, None))
    refused(lib.oct_grad_norm(x, 0, 1.0, 1.0, x, x, None))
    refused(lib.oct_grad_norm(x, 16, 1.0, 0.0, x, x, None))
    assert "max_norm" in L.last_error()
    assert lib.oct_grad_norm_blocks(0) == 0 and lib.oct_grad_norm_blocks(1) == 1 and lib.oct_grad_norm_blocks(1024) == 1
    assert lib.oct_grad_norm_blocks(1025) == 2 and lib.oct_grad_norm_blocks(2048 * 1024 + 1) == 2048
    assert lib.oct_grad_norm_blocks(1 << 30) == 2048

    refused(lib.oct_sgd_step_scaled(None, x, None, 16, 0.1, 0.0, 0.0, 1.0, 0, None, None, None))
    refused(lib.oct_sgd_step_scaled(x, None, None, 16, 0.1, 0.0, 0.0, 1.0, 0, None, None, None))
    refused(lib.oct_sgd_step_scaled(x, x, None, 0, 0.1, 0.0, 0.0, 1.0, 0, None, None, None))
    refused(lib.oct_sgd_step_scaled(x, x, None, 16, 0.1, 0.9, 0.0, 1.0, 0, None, None, None))
    assert "momentum" in L.last_error()


def test_fused_optimizers_refuse_cpu_parameters_and_unsupported_keywords(L):
    from retinal_oct_image_segmentation_via_deep_learning_amd import optim as O
    model = small_unet()
    for cls in (O.FusedAdam, O.FusedAdamW):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls(list(model.named_parameters()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        O.FusedSGD(list(model.named_parameters()), lr=0.1, max_grad_norm=1.0)
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"nesterov": True}):
        with pytest.raises(NotImplementedError):
            O.FusedAdam(list(model.named_parameters()), **kw)
    with pytest.raises(NotImplementedError):
        O.FusedSGD(list(model.named_parameters()), lr=0.1, nesterov=True)
    with pytest.raises(NotImplementedError):
        O.FusedAdam([{"params": list(model.parameters()), "lr": 0.1}])
    with pytest.raises(ValueError):
        O.FusedAdam(list(model.named_parameters()), betas=(0.9, 1.0))
    sig = inspect.signature(O.FusedAdam.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:9]] == \
        [("params", inspect._empty), ("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("weight_decay", 0.0),
         ("decoupled", False), ("max_grad_norm", None), ("no_decay", None)]
    wsig = inspect.signature(O.FusedAdamW.__init__).parameters
    assert wsig["weight_decay"].default == 1e-2 and "decoupled" not in wsig
    assert O.NO_DECAY_1D("x", torch.zeros(3)) and not O.NO_DECAY_1D("x", torch.zeros(3, 3))


def test_trainer_keywords_and_their_defaults():
    from retinal_oct_image_segmentation_via_deep_learning_amd import ddp
    sig = inspect.signature(ddp.DataParallelTrainer.__init__).parameters
    assert [(k, sig[k].default) for k in ("optimizer", "betas", "eps", "max_grad_norm", "no_decay")] == \
        [("optimizer", "sgd"), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("max_grad_norm", None), ("no_decay", None)]
    assert [(k, sig[k].default) for k in ("lr", "momentum", "weight_decay")] == [("lr", 0.01), ("momentum", 0.9), ("weight_decay", 0.0)]
    with pytest.raises(ValueError, match="optimizer"):
        ddp.DataParallelTrainer(small_unet(), optimizer="lion")
    assert hasattr(ddp.DataParallelTrainer, "state_dict") and hasattr(ddp.DataParallelTrainer, "load_state_dict")
