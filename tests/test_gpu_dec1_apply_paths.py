"""One bf16 training step of UNet(1, 8, 32) on the wide fixture (2 x 64 x 128) with and without the two full-resolution
BatchNorm-backward shortcuts of the last decoder block:

* `head_dl_off`: the head stores dlogits (16 B per pixel) and dec1.conv2's apply pass recomputes dA (oct_head_backward_dl +
  oct_head_bwd_apply) -- against the head storing dA and oct_bn_bwd_apply reading it back;
* `wgrad_apply_off`: dec1.conv1's weight gradient applies the BatchNorm backward on load and stores dY (oct_conv_wgrad with
  dy_coef + dy_out) -- against oct_bn_bwd_apply in front of it.

Both produce the bits of what they replace, so the whole dA / dY chain of the step is bit-identical: the loss and every
BatchNorm gamma / beta gradient must be EQUAL.  Convolution weight and bias gradients meet through fp32 atomics; they are held
to the bound of tests/test_gpu_fused_backward.py::test_training_step_with_and_without_the_fused_launches: a tenth of the
distance of the bf16 step from its fp32 parity-mode step.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))


def test_training_step_with_and_without_the_dec1_apply_shortcuts(golden_dir):
    from oracle.cases import ynet_case
    from retinal_oct_image_segmentation_via_deep_learning_amd import UNet
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    z = np.load(os.path.join(golden_dir, "unet_c8_f32_2x64x128_wide.npz"))
    in_ch, ncls, feat, b, h, w = (int(v) for v in z["meta"])
    model, x, t = ynet_case(UNet, int(z["seed"]), in_ch, ncls, feat, (b, h, w))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    x, t = x.cuda(), t.cuda()
    eng = model._engine
    L.lib()
    calls = []

    def step(dtype, head_off, wgrad_off):
        model.load_state_dict(state)
        model.set_compute_dtype(dtype)
        eng.head_dl_off, eng.wgrad_apply_off = head_off, wgrad_off
        loss = model.forward_backward(x, t)
        torch.cuda.synchronize()
        return loss[0].item(), {k: p.grad.detach().double().cpu().numpy() for k, p in model.named_parameters()}

    # which launches a step with both shortcuts takes, seen through the engine's own helpers
    orig_bn, orig_wg = eng._bn_backward, eng._wgrad
    eng._bn_backward = lambda *a, **k: (calls.append(("bn", k.get("head_dl") is not None)), orig_bn(*a, **k))[1]
    eng._wgrad = lambda *a, **k: (calls.append(("wgrad", k.get("dy_out") is not None)), orig_wg(*a, **k))[1]
    try:
        l_on, g_on = step("bf16", False, False)
    finally:
        del eng._bn_backward, eng._wgrad
    assert sum(1 for c in calls if c == ("bn", True)) == 1, "dec1.conv2 takes the dl8 route"
    assert sum(1 for c in calls if c == ("wgrad", True)) == 1, "dec1.conv1 applies on load and stores dY"
    l_off, g_off = step("bf16", True, True)
    l_h, g_h = step("bf16", False, True)     # each switch on its own
    l_w, g_w = step("bf16", True, False)
    _, g_f32 = step("f32", True, True)
    eng.head_dl_off = eng.wgrad_apply_off = False
    for what, (l, g) in {"both": (l_on, g_on), "head only": (l_h, g_h), "wgrad only": (l_w, g_w)}.items():
        assert l == l_off, (what, l, l_off)
        worst = 0.0
        for k in g_off:
            if "norm" in k:
                assert np.array_equal(g[k], g_off[k]), f"{what}: {k} differs (the dA / dY chain must be bit-identical)"
                continue
            yard, diff = rel_l2(g_off[k], g_f32[k]), rel_l2(g[k], g_off[k])
            worst = max(worst, diff / yard)
            assert diff < 0.1 * yard, (what, k, diff, yard)
        print(f"{what}: largest conv-gradient difference {worst:.2e} of the bf16-vs-f32 yardstick")
