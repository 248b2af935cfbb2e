"""Validation scoring on the cfg2 batch (32 x 512 x 1024 class maps, 8 classes): the one-vs-rest route that existed before the
streaming evaluator against `SegEvaluator`, with HIP events, warm-up and the median over the timed calls.

  oct_class_confusion_counts   the per-class kernel alone, on the same pair (zero + count + finish launches)
  SegEvaluator.update          one launch: C x C confusion matrix + thickness, added to the device state
  SegEvaluator.update_logits   the same from NHWC bf16 logits (arg-max inside the kernel, no class map)
  predict -> Metrics.evaluate  the whole per-batch call of the old route, UNet(1, 8) in eval mode, with its synchronisation,
                               against update_model (no synchronisation; the device is drained for the timing only)
each on piecewise-constant "layered" maps and on uniformly random ones, int64 and uint8, next to the bytes a call has to read
(268 MB int64 pair, 33.5 MB uint8 pair, 268 MB of bf16 logits + the target).  Prints a table and writes --out (JSON)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retinal_oct_image_segmentation_via_deep_learning_amd import Metrics, UNet, _lib as L  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.evaluation import SegEvaluator  # noqa: E402

HBM = 6.3e12   # bytes / s the chip streams


def layered(n, h, w, classes, gen, jitter):
    """device int64 class maps: per column `classes` bands along H, boundaries waving along W; the prediction's are moved"""
    base = torch.sort(torch.rand(n, classes - 1, 1, generator=gen) * h, dim=1).values
    phase = torch.rand(n, classes - 1, 1, generator=gen) * 6.28
    xs = torch.arange(w, dtype=torch.float32)[None, None, :]
    bt = base + 6.0 * torch.sin(xs / 40.0 + phase)
    bp = bt + torch.randint(-jitter, jitter + 1, bt.shape, generator=gen).float()
    yy = torch.arange(h, dtype=torch.float32, device="cuda")[None, :, None]
    out = []
    for b in (bt, bp):
        b = b.cuda()
        lab = torch.zeros(n, h, w, dtype=torch.int64, device="cuda")
        for k in range(classes - 1):
            lab += yy >= b[:, k][:, None, :]
        out.append(lab)
    return out


def median_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


def host_median_ms(fn, warmup, iters):
    """host clock around work that ends with the device drained"""
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-model", action="store_true", help="skip the predict -> evaluate / update_model comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    n, h, w, c = a.batch, a.height, a.width, a.classes
    npix = n * h * w
    gen = torch.Generator().manual_seed(1234)
    maps = {"layered": layered(n, h, w, c, gen, 3),
            "random": [torch.randint(0, c, (n, h, w), generator=gen).cuda() for _ in range(2)]}
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    oc, sc = torch.empty((c, 6), dtype=torch.int64, device="cuda"), torch.empty(48, dtype=torch.int64, device="cuda")
    rows = []

    def row(name, kind, dtype, nbytes, us, **extra):
        r = dict(case=name, maps=kind, dtype=dtype, bytes=nbytes, us=round(us, 1), gb_per_s=round(nbytes / us / 1e3, 1),
                 of_hbm=round(nbytes / (us * 1e-6) / HBM, 3), **extra)
        rows.append(r)
        print(f"{name:34s} {kind:8s} {dtype:6s} {nbytes / 1e6:7.1f} MB {us:9.1f} us {r['gb_per_s']:8.1f} GB/s {r['of_hbm']:6.3f} of 6.3 TB/s", flush=True)

    for kind, (t64, p64) in maps.items():
        agree = float((t64 == p64).float().mean())
        for dtype, (t, p), elem in (("int64", (t64, p64), 2), ("uint8", (t64.to(torch.uint8), p64.to(torch.uint8)), 0)):
            nbytes = 2 * npix * t.element_size()
            us_old = median_us(lambda: lib.oct_class_confusion_counts(t.data_ptr(), p.data_ptr(), elem, npix, c, oc.data_ptr(),
                                                                      sc.data_ptr(), st), a.warmup, a.iters)
            row("oct_class_confusion_counts", kind, dtype, nbytes, us_old, agreement=round(agree, 4))
            ev = SegEvaluator(c)
            us_new = median_us(lambda: ev.update(t, p), a.warmup, a.iters)
            row("SegEvaluator.update", kind, dtype, nbytes, us_new, vs_one_vs_rest=round(us_new / us_old, 3))
            # the two routes count the same pixels
            m = SegEvaluator(c).update(t, p).compute()
            assert (m["counts"] == Metrics.evaluate(t, p, classes=c)["counts"]).all()
            # NHWC bf16 logits whose arg-max is the prediction map
            lg = torch.randn(n, h, w, c, device="cuda", dtype=torch.bfloat16)
            lg.scatter_(3, p64[..., None], 8.0)
            evl = SegEvaluator(c)
            us_lg = median_us(lambda: evl.update_logits(t, lg, "nhwc"), a.warmup, a.iters)
            row("SegEvaluator.update_logits bf16", kind, dtype, lg.numel() * 2 + npix * t.element_size(), us_lg)
            assert (SegEvaluator(c).update_logits(t, lg, "nhwc").compute()["confusion"] == m["confusion"]).all()
            del lg
    if not a.no_model:
        torch.manual_seed(0)
        model = UNet(1, c, init_features=32, compute_dtype="bf16").cuda().eval()
        x = torch.randn(n, 1, h, w, generator=gen).cuda()
        t = maps["layered"][0]
        ms_fwd = host_median_ms(lambda: model.predict(x), 2, 5)
        ms_old = host_median_ms(lambda: Metrics.evaluate(t, model.predict(x), classes=c), 2, 5)
        ev = SegEvaluator(c)
        ms_new = host_median_ms(lambda: ev.update_model(model, x, t), 2, 5)
        for name, ms in (("predict", ms_fwd), ("predict -> Metrics.evaluate", ms_old), ("update_model", ms_new)):
            rows.append(dict(case=name, maps="layered", dtype="int64", ms=round(ms, 3)))
            print(f"{name:34s} UNet(1,{c}) eval, {n} x {h} x {w}: {ms:9.3f} ms per batch (host clock, device drained)", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"shape": [n, h, w], "classes": c, "warmup": a.warmup, "iters": a.iters, "device": torch.cuda.get_device_name(0),
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
