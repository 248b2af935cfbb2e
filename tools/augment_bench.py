"""Paired augmentation at the cfg2 batch (32 x 1 x 512 x 1024 uint8 B-scans + uint8 class map + fp32 pixel-weight map -> bf16
image + int64 target + fp32 weight map), with HIP events around a loop of launches, warm-up, and at least --min-seconds of timed
work per line:

  (a) geometry only   flip + rotation + scale + shift, different per sample
  (b) + elastic       control grid of pitch 32, sigma 4 px
  (c) + gamma
  (d) + noise         speckle + additive: one Philox call and one Box-Muller pair per two pixels
  (e) device copy     a plain copy moving the same bytes: the floor
  (f) torch           affine_grid + grid_sample (bilinear: image and weight map; nearest: labels), a gamma pass, randn_like twice
  PairAugmenter       (d) through the public call, parameters drawn on the host, on the host clock (device drained per call)

(a) - (d) time oct_augment_pair alone, its parameters already on the device.  Bytes per output pixel: reads 1 (image) + 1 (label)
+ 4 (weight), writes 2 + 8 + 4: 20.  Unless --step-ms is given the cfg2 headline is measured first, by bench.py in a child
process, and every line is also stated as a share of that step.  Prints a table and writes --out (JSON)."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L  # noqa: E402
from retinal_oct_image_segmentation_via_deep_learning_amd import augment as A  # noqa: E402

HBM = 6.3e12   # bytes / s the chip streams
BYTES_PER_PIXEL = {"read": 1 + 1 + 4, "write": 2 + 8 + 4}


def headline_ms(steps, warmup):
    """ms per step of the cfg2 headline line, measured by bench.py in a fresh child process"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         capture_output=True, text=True, cwd=ROOT)
    for line in reversed(res.stdout.splitlines()):
        if line.startswith("{"):
            return float(json.loads(line)["ms_per_step"])
    raise RuntimeError("bench.py printed no result line:\n" + res.stdout[-2000:] + res.stderr[-2000:])


def timed_us(fn, warmup, min_seconds):
    """(us per call, calls timed): device events around a loop long enough for min_seconds of work"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        fn()
    b.record()
    torch.cuda.synchronize()
    est = max(a.elapsed_time(b) / 10 * 1e-3, 1e-6)
    n = max(20, int(math.ceil(min_seconds / est)))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--step-ms", type=float, default=None, help="cfg2 step time to state the shares against (default: measure it)")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    a = ap.parse_args()
    step_ms = a.step_ms if a.step_ms is not None else headline_ms(a.bench_steps, a.bench_warmup)   # before this process opens the GPU
    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    n, h, w = a.batch, a.height, a.width
    pixels = n * h * w
    per_pixel = BYTES_PER_PIXEL["read"] + BYTES_PER_PIXEL["write"]
    nbytes = per_pixel * pixels
    gen = torch.Generator().manual_seed(1234)
    x = torch.randint(0, 256, (n, 1, h, w), generator=gen, dtype=torch.uint8).cuda()
    t = torch.randint(0, 8, (n, h, w), generator=gen, dtype=torch.uint8).cuda()
    wt = torch.rand((n, h, w), generator=gen).cuda()
    lib, st = L.lib(), torch.cuda.current_stream().cuda_stream
    kw = dict(hflip=0.5, rotate_deg=10.0, scale=(0.9, 1.1), translate=(0.02, 0.05), gain=(1 / 255, 1 / 255), clamp=(0.0, 1.0),
              label_fill=255, seed=1)
    stages = [("(a) geometry only", {}),
              ("(b) + elastic", dict(elastic_pitch=32, elastic_sigma_px=4.0)),
              ("(c) + gamma", dict(elastic_pitch=32, elastic_sigma_px=4.0, gamma=(0.8, 1.25))),
              ("(d) + noise", dict(elastic_pitch=32, elastic_sigma_px=4.0, gamma=(0.8, 1.25), speckle=0.1, noise=0.02))]
    rows = []

    def row(name, us, calls, **extra):
        r = dict(case=name, us=round(us, 1), calls=calls, gb_per_s=round(nbytes / us / 1e3, 1), of_hbm=round(nbytes / (us * 1e-6) / HBM, 3),
                 share_of_step=round(us * 1e-3 / step_ms, 5), **extra)
        rows.append(r)
        print(f"{name:28s} {us:9.1f} us  {r['gb_per_s']:8.1f} GB/s  {r['of_hbm']:6.3f} of 6.3 TB/s  {100 * r['share_of_step']:6.3f} % of the step "
              + " ".join(f"{k}={v}" for k, v in extra.items()), flush=True)

    x_out = torch.empty((n, 1, h, w), dtype=torch.bfloat16, device="cuda")
    t_out = torch.empty((n, h, w), dtype=torch.int64, device="cuda")
    w_out = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    us_of = {}
    for name, extra in stages:
        aug = A.PairAugmenter(**kw, **extra)
        p = aug.draw(n, (h, w))
        words = torch.from_numpy(p.words().view(np.int32)).cuda()
        disp = torch.from_numpy(p.disp).cuda() if p.disp is not None else None
        d = L.AugmentDesc(n, 1, h, w, h, w, L.AUG_U8, L.AUG_BF16, L.AUG_LABEL_CLASS_U8, 1, p.flags, p.pitch or 0, 1, 0, 0, 0, 0.0, 0, 255)

        def launch():
            L.check(lib.oct_augment_pair(C.byref(d), x.data_ptr(), t.data_ptr(), wt.data_ptr(), words.data_ptr(), L.ptr(disp),
                                         x_out.data_ptr(), t_out.data_ptr(), w_out.data_ptr(), st), "oct_augment_pair")
        us, calls = timed_us(launch, a.warmup, a.min_seconds)
        us_of[name] = us
        row(name, us, calls, ignored_share=round(float((t_out == 255).float().mean()), 4))

    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    us, calls = timed_us(lambda: dst.copy_(src), a.warmup, a.min_seconds)
    row("(e) device copy", us, calls)
    del src, dst

    theta = torch.tensor([[[0.98, 0.05, 0.01], [-0.05, 0.98, 0.02]]], device="cuda").repeat(n, 1, 1)

    def torch_composition():
        grid = F.affine_grid(theta, (n, 1, h, w), align_corners=False)
        both = F.grid_sample(torch.cat([x.float(), wt[:, None]], 1), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        lab = F.grid_sample(t[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False).to(torch.int64)
        img = (both[:, :1] * (1 / 255)).clamp_(0, 1).pow_(1.1)
        img = img * (1 + 0.1 * torch.randn_like(img)) + 0.02 * torch.randn_like(img)
        return img.clamp_(0, 1).to(torch.bfloat16), lab, both[:, 1]
    us, calls = timed_us(torch_composition, a.warmup, a.min_seconds)
    row("(f) torch composition", us, calls, d_over_f=round(us_of["(d) + noise"] / us, 4))

    # the public call: parameters drawn on the host per call (the elastic nodes are the bulk), one pinned upload, one launch
    aug = A.PairAugmenter(**kw, **stages[-1][1])
    ts = []
    for i in range(a.warmup + 20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug(x, target=t, pixel_weight=wt)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ts.append(((t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6))
    host_us, total_us = (float(np.median([v[k] for v in ts])) for k in (0, 1))
    row("PairAugmenter call (d)", total_us, len(ts), host_us=round(host_us, 1))

    d_exceeds_f = us_of["(d) + noise"] > rows[5]["us"]
    print(f"(d) {'EXCEEDS' if d_exceeds_f else 'does not exceed'} (f)", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"shape": [n, 1, h, w], "device": torch.cuda.get_device_name(0), "min_seconds": a.min_seconds, "warmup": a.warmup,
                   "bytes_per_pixel": dict(BYTES_PER_PIXEL, total=per_pixel), "bytes_per_call": nbytes,
                   "cfg2_step_ms": round(step_ms, 3), "cfg2_step_from": "--step-ms" if a.step_ms is not None else "bench.py in this run",
                   "d_exceeds_f": bool(d_exceeds_f), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
