"""Score evaluator on the cfg2 validation batch as the binary head sees it (32 x 8 x 512 x 1024 logits + the uint8 target), with
HIP events, warm-up and the median over the timed calls; all launches of a call are inside the events.

  ScoreEvaluator.update NCHW fp32   one launch: the [2][65536] key histogram of every channel, added to the device state
  oct_bce_loss_forward (mask only)  the yardstick for ONE pass over the same bytes: what predict_mask runs on the same buffers
                                    (it also writes the uint8 mask)
  ScoreEvaluator.update NHWC bf16   the logits networks' own layout: oct_nhwc_to_nchw to planar fp32, then the same launch
  logits -> update_model            UNet(1, 8) in eval mode on the host clock, against model.logits(x) alone
on a smooth field (what logits look like: neighbouring pixels share keys) and an i.i.d. normal one (up to 64 distinct keys per
wave), next to the one-pass byte floor (4 B score + 1 B target per element).  Prints a table and writes --out (JSON)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retinal_oct_image_segmentation_via_deep_learning_amd import UNet, _lib as L  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd.evaluation import ScoreEvaluator  # noqa: E402

HBM = 6.3e12   # bytes / s the chip streams


def smooth_logits(n, c, h, w, gen):
    """device fp32 logits: per plane two wide blobs on a background of -4, plus a fine ripple"""
    yy = torch.arange(h, dtype=torch.float32, device="cuda")[None, None, :, None]
    xx = torch.arange(w, dtype=torch.float32, device="cuda")[None, None, None, :]
    out = torch.full((n, c, h, w), -4.0, device="cuda")
    for _ in range(2):
        cy = (torch.rand(n, c, 1, 1, generator=gen) * h).cuda()
        cx = (torch.rand(n, c, 1, 1, generator=gen) * w).cuda()
        r = (40.0 + torch.rand(n, c, 1, 1, generator=gen) * 120.0).cuda()
        out += 8.0 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return out + 0.05 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)


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
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-model", action="store_true", help="skip the logits -> update_model comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "score_bench needs a GPU"
    n, h, w, c = a.batch, a.height, a.width, a.channels
    elems = n * c * h * w
    floor = 5 * elems                                   # fp32 score + uint8 target, read once
    gen = torch.Generator().manual_seed(1234)
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    rows, us_of = [], {}

    def row(name, field, nbytes, us, **extra):
        r = dict(case=name, field=field, bytes=nbytes, us=round(us, 1), gb_per_s=round(nbytes / us / 1e3, 1),
                 of_hbm=round(nbytes / (us * 1e-6) / HBM, 3), **extra)
        rows.append(r)
        print(f"{name:36s} {field:7s} {nbytes / 1e6:7.1f} MB {us:9.1f} us {r['gb_per_s']:8.1f} GB/s {r['of_hbm']:6.3f} of 6.3 TB/s "
              + " ".join(f"{k}={v}" for k, v in extra.items()), flush=True)

    for field in ("smooth", "random"):
        lg = smooth_logits(n, c, h, w, gen) if field == "smooth" else 3.0 * torch.randn(n, c, h, w, device="cuda")
        t = ((lg + torch.randn_like(lg)) > 0.5).to(torch.uint8)
        ev = ScoreEvaluator(c)
        us = median_us(lambda: ev.update(t, lg), a.warmup, a.iters)
        m = ScoreEvaluator(c).update(t, lg).compute()
        occupied = int((ScoreEvaluator(c).update(t, lg).state[:c * 2 * 65536].view(c, 2, 65536).sum(dim=1) > 0).sum(dim=1).max())
        row("ScoreEvaluator.update NCHW fp32", field, floor, us, occupied_keys_max=occupied,
            auc0=round(float(m["auc"][0]), 6), bracket0=float(m["auc_hi"][0] - m["auc_lo"][0]))
        us_of[field] = us
        # one pass over the same buffers: the mask-only launch of predict_mask (reads 4 B, writes 1 B per element)
        mask = torch.empty((n, c, h, w), dtype=torch.uint8, device="cuda")
        desc = L.HeadDesc(L.DT_F32, n, h, w, 1, c)
        us_mask = median_us(lambda: lib.oct_bce_loss_forward(C.byref(desc), L.SEG_NCHW, lg.data_ptr(), None, None, None, 0, 0, 0,
                                                             0.0, mask.data_ptr(), None, st), a.warmup, a.iters)
        assert bool((mask.bool() == (lg >= 0)).all())
        row("oct_bce_loss_forward mask only", field, floor, us_mask, update_over_mask=round(us / us_mask, 2))
        # the counts at 0.5 are those of the mask
        assert int(m["counts"][:, 0, 2].sum()) == int(mask.sum())
        del mask
        nh = lg.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
        evn = ScoreEvaluator(c)
        us_nh = median_us(lambda: evn.update(t, nh, "nhwc"), a.warmup, a.iters)
        row("ScoreEvaluator.update NHWC bf16", field, 2 * elems + elems, us_nh, over_nchw=round(us_nh / us, 2))
        del nh, lg, t
    ratio = us_of["random"] / us_of["smooth"]
    print(f"random / smooth: {ratio:.2f}", flush=True)
    if not a.no_model:
        torch.manual_seed(0)
        model = UNet(1, c, init_features=32, compute_dtype="bf16").cuda().eval()
        x = torch.randn(n, 1, h, w, generator=gen).cuda()
        t = (torch.rand(n, c, h, w, device="cuda") < 0.1).to(torch.uint8)
        ms_fwd = host_median_ms(lambda: model.logits(x), 2, 5)
        ev = ScoreEvaluator(c)
        ms_new = host_median_ms(lambda: ev.update_model(model, x, t), 2, 5)
        for name, ms in (("logits", ms_fwd), ("update_model", ms_new)):
            rows.append(dict(case=name, field="model", ms=round(ms, 3)))
            print(f"{name:36s} UNet(1,{c}) eval, {n} x {h} x {w}: {ms:9.3f} ms per batch (host clock, device drained)", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"shape": [n, c, h, w], "warmup": a.warmup, "iters": a.iters, "device": torch.cuda.get_device_name(0),
                       "one_pass_floor_bytes": floor, "random_over_smooth": round(ratio, 3), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
