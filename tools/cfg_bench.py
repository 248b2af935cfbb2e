"""Throughput of the parity configurations (not the bench line), bf16, training step = fwd + loss + bwd + SGD(momentum).

  cfg1 BioNet UNet(1,2) 4x256x256 and 32x256x256: forward_backward + FusedSGD (engine network)
  cfg4 AttU_Net(1,3) 16x496x768, ReLayNet(1,10) 16x496x768, MGUNet_2(1,11) 16x496x768, two ways each, alternating in one
  process (same seeds, same inputs):
    torch  -- F.cross_entropy(model(x), t) + torch.optim.SGD: NCHW fp32 logits, ATen log_softmax / nll_loss
    fused  -- model.forward_backward(x, t) + FusedSGD: the loss kernels on the NHWC logits (losses.py, csrc/seg_loss.hip)

usage: cfg_bench.py [steps] [rounds]     CFG_ONLY=1 / 4 / relaynet / mgunet2 / unet runs one group.
CFG_PROFILE=1: only the fused cfg4 step, 3 warm-up steps + 1 (for a rocprofv3 --kernel-trace --stats pass).
CFG_WEIGHTED=1: the weighted loss in the cfg4 pairs and the profile step -- class weights w (uniform in [0.25, 4]) and
  ignore_index k = 255 on 20 % of the labels:
    torch  -- F.cross_entropy(model(x), t, weight=w, ignore_index=k) + torch.optim.SGD
    fused  -- model.forward_backward(x, t, class_weight=w, ignore_index=k) + FusedSGD (oct_seg_loss_*_weighted)
  and, as group "unet" (only when named: CFG_ONLY=unet), UNet(1,8) at the headline shape 32x512x1024: the weighted step, which
  leaves the fused head, against the unweighted fused-head step of the same build, alternating.
CFG_ONLY=binary (only when named): the binary head, AttU_Net(1,1) 16x496x768 against a random uint8 mask, alternating:
    torch  -- F.binary_cross_entropy_with_logits(model(x), t.float()) + torch.optim.SGD
    fused  -- model.forward_backward_binary(x, t) + FusedSGD (oct_bce_loss_* on the NHWC logits)
  with CFG_PROFILE=1 only the fused binary step, 3 warm-up steps + 1."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.ReLayNet_2017 import ReLayNet  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.BioNet_2020 import UNet as BioUNet  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.MGUNet_2021 import MGUNet_2  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Layers_Segment.SD_Layer_Net.unet import AttU_Net  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.SOTAS.Lesions_Segment.YNet_2022 import UNet  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.optim import FusedSGD  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
WARMUP = 8     # the autograd-driven networks reach their steady state after ~8 steps (bench.py)
WEIGHTED = bool(os.environ.get("CFG_WEIGHTED"))
IGNORE = 255
g = torch.Generator().manual_seed(1234)


def weighted_options(t, ncls):
    """(labels with 20 % set to IGNORE, class weights on the device); the generator advances only in weighted mode"""
    w = (0.25 + 3.75 * torch.rand(ncls, generator=g)).cuda()
    t = torch.where(torch.rand(t.shape, generator=g).cuda() < 0.2, torch.full_like(t, IGNORE), t)
    return t, w


def stepper(model, x, t, fused, w=None, k=None):
    model.cuda().train()
    kw = {} if w is None else dict(class_weight=w, ignore_index=k)
    if fused:
        opt = FusedSGD(list(model.named_parameters()), lr=0.01, momentum=0.9)

        def step():
            model.forward_backward(x, t, **kw)
            opt.step()
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
        tkw = {} if w is None else dict(weight=w, ignore_index=k)

        def step():
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(model(x), t, **tkw).backward()
            opt.step()
    return step


def binary_stepper(model, x, t, fused):
    model.cuda().train()
    if fused:
        opt = FusedSGD(list(model.named_parameters()), lr=0.01, momentum=0.9)

        def step():
            model.forward_backward_binary(x, t)
            opt.step()
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
        tf = t.float()      # converted once, outside the step: the torch path is not charged for it

        def step():
            opt.zero_grad(set_to_none=True)
            F.binary_cross_entropy_with_logits(model(x), tf).backward()
            opt.step()
    return step


def timed(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def run(name, model, x, t):
    """engine network: forward_backward + FusedSGD only"""
    step = stepper(model, x, t, True)
    for _ in range(3):
        step()
    dt = timed(step, steps)
    print(f"{name}: {dt * 1e3:.2f} ms/step, {x.shape[0] / dt:.1f} B-scans/s, peak memory "
          f"{torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


def pair(name, make, x, t, w=None, k=None, binary=False):
    """the torch-CE path and the fused path of two identically seeded models, timed in alternating rounds"""
    torch.manual_seed(0)
    st_torch = binary_stepper(make(), x, t, False) if binary else stepper(make(), x, t, False, w, k)
    torch.manual_seed(0)
    st_fused = binary_stepper(make(), x, t, True) if binary else stepper(make(), x, t, True, w, k)
    for _ in range(WARMUP):
        st_torch()
        st_fused()
    ms = {"torch": [], "fused": []}
    for _ in range(rounds):
        ms["torch"].append(timed(st_torch, steps) * 1e3)
        ms["fused"].append(timed(st_fused, steps) * 1e3)
    a, b = statistics.median(ms["torch"]), statistics.median(ms["fused"])
    tag = "weighted " if w is not None else ""
    lname, fname = ("BCE", "forward_backward_binary") if binary else ("CE", "forward_backward")
    print(f"{name}: torch {tag}{lname} + SGD {a:.2f} ms/step, {tag}{fname} + FusedSGD {b:.2f} ms/step "
          f"({a - b:+.2f} ms, {a / b:.3f}x; medians of {rounds} rounds x {steps} steps; "
          f"rounds torch {['%.2f' % v for v in ms['torch']]} fused {['%.2f' % v for v in ms['fused']]})", flush=True)


ONLY = os.environ.get("CFG_ONLY", "")
torch.manual_seed(0)
if ONLY == "binary":
    x = torch.randn(16, 1, 496, 768, generator=g).cuda()
    t = (torch.rand(16, 1, 496, 768, generator=g) < 0.3).to(torch.uint8).cuda()
    if os.environ.get("CFG_PROFILE"):
        torch.manual_seed(0)
        step = binary_stepper(AttU_Net(1, 1), x, t, True)
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        print("binary fused: 4 steps done")
    else:
        pair("binary AttU_Net(1,1) 16x496x768", lambda: AttU_Net(1, 1), x, t, binary=True)
    sys.exit(0)
if os.environ.get("CFG_PROFILE"):
    x = torch.randn(16, 1, 496, 768, generator=g).cuda()
    t = torch.randint(0, 3, (16, 496, 768), generator=g).cuda()
    w = None
    if WEIGHTED:
        t, w = weighted_options(t, 3)
    torch.manual_seed(0)
    step = stepper(AttU_Net(1, 3), x, t, True, w, IGNORE if WEIGHTED else None)
    for _ in range(4):
        step()
    torch.cuda.synchronize()
    print(f"cfg4 fused{' weighted' if WEIGHTED else ''}: 4 steps done")
    sys.exit(0)
if ONLY == "unet":
    # the weighted step of an engine network (NCHW fp32 logits, the loss kernels, the generic 1x1 head backward) against the
    # fused-head step it leaves, same model, same labels apart from the ignored ones
    x = torch.randn(32, 1, 512, 1024, generator=g).cuda()
    t = torch.randint(0, 8, (32, 512, 1024), generator=g).cuda()
    tw, w = weighted_options(t, 8)
    torch.manual_seed(0)
    st_plain = stepper(UNet(1, 8), x, t, True)
    torch.manual_seed(0)
    st_w = stepper(UNet(1, 8), x, tw, True, w, IGNORE)
    for _ in range(3):
        st_plain()
        st_w()
    ms = {"plain": [], "weighted": []}
    for _ in range(rounds):
        ms["plain"].append(timed(st_plain, steps) * 1e3)
        ms["weighted"].append(timed(st_w, steps) * 1e3)
    a, b = statistics.median(ms["plain"]), statistics.median(ms["weighted"])
    print(f"UNet(1,8) 32x512x1024: fused head {a:.2f} ms/step, weighted loss {b:.2f} ms/step ({b - a:+.2f} ms, {b / a:.3f}x; "
          f"medians of {rounds} rounds x {steps} steps; rounds fused head {['%.2f' % v for v in ms['plain']]} "
          f"weighted {['%.2f' % v for v in ms['weighted']]})", flush=True)
    sys.exit(0)
if ONLY in ("", "1"):
    x = torch.randn(4, 1, 256, 256, generator=g).cuda(); t = torch.randint(0, 2, (4, 256, 256), generator=g).cuda()
    run("cfg1 BioNet UNet(1,2) 4x256x256", BioUNet(1, 2), x, t)
    x = torch.randn(32, 1, 256, 256, generator=g).cuda(); t = torch.randint(0, 2, (32, 256, 256), generator=g).cuda()
    run("     BioNet UNet(1,2) 32x256x256", BioUNet(1, 2), x, t)
for key, name, make, ncls in (("4", "cfg4 AttU_Net(1,3) 16x496x768", lambda: AttU_Net(1, 3), 3),
                              ("relaynet", "ReLayNet(1,10) 16x496x768", lambda: ReLayNet(1, 10), 10),
                              ("mgunet2", "MGUNet_2(1,11) 16x496x768", lambda: MGUNet_2(1, 11), 11)):
    if ONLY in ("", key):
        x = torch.randn(16, 1, 496, 768, generator=g).cuda()
        t = torch.randint(0, ncls, (16, 496, 768), generator=g).cuda()
        if WEIGHTED:
            pair(name, make, x, *weighted_options(t, ncls), IGNORE)
        else:
            pair(name, make, x, t)
        torch.cuda.empty_cache()
