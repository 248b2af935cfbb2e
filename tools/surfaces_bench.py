"""Times of the layer-surface entry points on the MI355X at the cfg2 batch, 32 x 512 x 1024, K = 9 ordered classes, on wavy
retinal-layer bands with 5 % of the labels replaced uniformly at random:
  extract_none / extract_1 / extract_3   LayerSurfaces.extract of the uint8 map with max_step = None, 1, 3
  extract_scores_1                       LayerSurfaces.extract_scores of fp32 NCHW scores, max_step = 1
  paint                                  LayerSurfaces.paint of the uint8 map from its surfaces
  evaluator_update                       SurfaceEvaluator.update of two surface tensors

HIP events around a loop of calls, warm-up, the loop sized so that every sample lasts at least --min-sample-ms and the samples
of an entry together at least half a second; median, min and max over the samples, per call.  Next to each time:
  floor_ms      the bytes the operation must move -- its input once, its output once -- over the achievable HBM rate
                (--hbm-tbps, 6.3 TB/s); launched_ms the same for the bytes the launch sequence moves, workspace included: with a
                step limit N is written and read (4 + 4 bytes per cell of (K-1) W (H+1)) and P written (1 byte)
  step_us       with a step limit: the whole call over the W - 1 dependent steps of a search workgroup -- an upper bound of one
                step (cost pass and walk back are inside it; the kernels' own times: profiles/README.md)
  host_s        tests/surf_ref.py on the same input: timed on the first --host-images images and scaled to the batch (images
                are independent); the device result on those images is compared with it, ==, before anything is timed

    python tools/surfaces_bench.py [--out profiles/surfaces_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from distance_bench import timed  # noqa: E402  (tools/ is on the path of a script run from it)


def layer_bands(rng, images, h, w, k, noise):
    """(uint8 map [images, h, w], fp32 scores [images, k, h, w]): k wavy bands, `noise` of the labels replaced"""
    import surf_ref
    x = np.arange(w)
    maps = []
    for _ in range(images):
        base = np.sort(rng.uniform(0.1, 0.9, size=k - 1)) * h
        wave = rng.uniform(0.02, 0.06) * h * np.sin(2 * np.pi * (x / w * rng.uniform(0.5, 2.0) + rng.uniform()))
        cuts = np.maximum.accumulate(np.clip(np.rint(base[:, None] + wave[None, :]), 0, h).astype(np.int64), axis=0)
        maps.append(surf_ref.band_map(h, w, cuts))
    clean = np.stack(maps)
    m = np.where(rng.random(clean.shape) < noise, rng.integers(0, k, size=clean.shape), clean).astype(np.uint8)
    z = rng.normal(size=(images, k, h, w)).astype(np.float32)
    z += 2.0 * (np.arange(k).reshape(1, -1, 1, 1) == m[:, None]).astype(np.float32)
    return m, z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--min-sample-ms", type=float, default=50.0)
    ap.add_argument("--host-images", type=int, default=2, help="images surf_ref is timed (and the device checked) on; 0: skip")
    ap.add_argument("--hbm-tbps", type=float, default=6.3, help="the achievable HBM rate the floors are taken at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surfaces_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surfaces_bench needs a GPU: a time taken anywhere else says nothing")
    import surf_ref
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation, surfaces

    b, h, w, k = a.images, a.height, a.width, a.classes
    order = list(range(k))
    m, z = layer_bands(np.random.default_rng(0), b, h, w, k, a.noise)
    mt, zt = torch.from_numpy(m).cuda(), torch.from_numpy(z).cuda()
    ex = {step: surfaces.LayerSurfaces(k, order, max_step=step, max_workspace_bytes=1 << 30) for step in (None, 1, 3)}
    surf = {step: ex[step].extract(mt) for step in ex}
    surf_scores = ex[1].extract_scores(zt)

    host = {}
    nh = min(a.host_images, b)
    for name, fn in (("extract_none", lambda: surf_ref.extract(m[:nh], order, k, None)),
                     ("extract_1", lambda: surf_ref.extract(m[:nh], order, k, 1)),
                     ("extract_3", lambda: surf_ref.extract(m[:nh], order, k, 3)),
                     ("extract_scores_1", lambda: surf_ref.extract_scores(z[:nh], order, 1)),
                     ("paint", lambda: surf_ref.paint(surf[1][:nh].cpu().numpy(), order, h)),
                     ("evaluator_update", lambda: surf_ref.error_state(surf[None][:nh].cpu().numpy(), surf[1][:nh].cpu().numpy()))):
        if nh == 0:
            break
        t0 = time.perf_counter()
        want = fn()
        host[name] = round((time.perf_counter() - t0) * b / nh, 3)
        got = {"extract_none": surf[None], "extract_1": surf[1], "extract_3": surf[3], "extract_scores_1": surf_scores}.get(name)
        if got is not None and not np.array_equal(got[:nh].cpu().numpy(), want):
            raise SystemExit(f"{name}: the device result differs from surf_ref on the first {nh} images")

    cells = b * (k - 1) * w * (h + 1)
    surf_bytes = 4 * b * (k - 1) * w
    rate = a.hbm_tbps * 1e12
    ev = evaluation.SurfaceEvaluator(k - 1)
    painted = torch.empty_like(mt)
    ops = {   # name: (call, bytes that must move, bytes the launches move)
        "extract_none": (lambda: ex[None].extract(mt), mt.numel() + surf_bytes, mt.numel() + surf_bytes),
        "extract_1": (lambda: ex[1].extract(mt), mt.numel() + surf_bytes, mt.numel() + 9 * cells + 2 * surf_bytes),
        "extract_3": (lambda: ex[3].extract(mt), mt.numel() + surf_bytes, mt.numel() + 9 * cells + 2 * surf_bytes),
        "extract_scores_1": (lambda: ex[1].extract_scores(zt), 4 * zt.numel() + surf_bytes, 4 * zt.numel() + 9 * cells + 2 * surf_bytes),
        "paint": (lambda: ex[1].paint(mt, surf[1], out=painted), 2 * mt.numel() + surf_bytes, 2 * mt.numel() + surf_bytes * -(-h // 64)),
        "evaluator_update": (lambda: ev.update(surf[None], surf[1]), 2 * surf_bytes, 2 * surf_bytes),
    }
    res = {"shape": [b, h, w], "classes": k, "noise": a.noise, "warmup": a.warmup, "min_sample_ms": a.min_sample_ms,
           "hbm_tbps": a.hbm_tbps, "workspace_bytes_per_image": 5 * cells // b, "host_images": nh, "ops": {}}
    for name, (call, must, launched) in ops.items():
        r = timed(call, a.warmup, a.samples, a.min_sample_ms)
        r["bytes"] = int(must)
        r["floor_ms"] = round(must / rate * 1e3, 4)
        r["times_floor"] = round(r["ms_median"] / r["floor_ms"], 1)
        r["launched_ms"] = round(launched / rate * 1e3, 4)
        if name in host:
            r["host_s"] = host[name]
        res["ops"][name] = r
        print(name, r, flush=True)
    for name in ("extract_1", "extract_3", "extract_scores_1"):
        r = res["ops"][name]
        r["step_us"] = round(r["ms_median"] / (w - 1) * 1e3, 3)
    res["mean_abs_shift_px"] = {f"step_{s}": round(float((surf[s] - surf[None]).abs().float().mean()), 4) for s in (1, 3)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
