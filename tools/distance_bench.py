"""Times of the distance-map entry points on the MI355X at the cfg2 batch, 32 x 512 x 1024, uint8 and int64 labels:
  weight      "boundary" -> gaussian weight map, fp32 (DistanceWeightMap: the training-step path)
  boundary    "boundary" -> int32 squared distances (squared_distance)
  classes9    nine ("class", c) planes -> int32
  signed9     the signed map of nine classes, fp32 (signed_distance)
on three inputs -- "bands6": six wavy retinal-layer bands in nine declared classes (tests/dt_ref.wavy_bands), "noise3": uniform
3-class noise, "corner": one site per image, in its first pixel, which is the walk's worst case (a pixel walks its whole
distance along the row before it stops): recorded so that the bound is known.

HIP events around a loop of calls, warm-up, the loop sized so that every sample lasts at least --min-sample-ms and the samples
of an entry together at least half a second; median, min and max over the samples, per call.  Next to each time stands the
floor: the bytes the launch sequence must move divided by a device copy rate measured in the same run (a 256 MiB copy, read +
write counted).

Bytes per pixel of the sequences as they are launched, per g plane (a plane of the output; two per class of the signed map):
  mask 1 read (the map as bytes; the boundary rule's neighbours come from the cache), dist 2 written (g, uint16), rows 2 read and
  4 written: 9 per plane; the signed map reads the class byte in both of its phases and writes one fp32 for two g planes:
  2 * 5 + 2 + 4 = 16 per class.  An int64 map is narrowed once: + 8 read + 1 written.  The masks (1/8 byte per pixel and plane,
  written and read) and the table (L2-resident) are not counted.

The host baseline it replaces: scipy.ndimage.distance_transform_edt per image and plane on the CPU (the site sets are given,
not timed) plus the upload of the fp32 result; absent where scipy is.

    python tools/distance_bench.py [--out profiles/distance_bench.json]
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

OPS = ("weight", "boundary", "classes9", "signed9")
G_PLANE_BYTES, SIGNED_CLASS_BYTES, NARROW_BYTES = 9, 16, 9


def bytes_per_pixel(op, dtype, classes):
    b = {"weight": G_PLANE_BYTES, "boundary": G_PLANE_BYTES, "classes9": G_PLANE_BYTES * classes,
         "signed9": SIGNED_CLASS_BYTES * classes}[op]
    return b + (NARROW_BYTES if dtype == "int64" else 0)


def inputs(kind, shape, rng):
    import dt_ref
    if kind == "bands6":
        return dt_ref.wavy_bands(rng, shape, 6)
    if kind == "noise3":
        return rng.integers(0, 3, size=shape)
    m = np.zeros(shape, dtype=np.int64)
    m[:, 0, 0] = 1
    return m


def timed(fn, warmup, samples, min_sample_ms):
    """per-call milliseconds: `samples` event-timed loops of `inner` calls each"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    once = max(e0.elapsed_time(e1), 1e-3)
    inner = int(min(2000, max(1, np.ceil(max(min_sample_ms, 500.0 / samples) / once))))
    times = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / inner)
    return {"ms_median": round(float(np.median(times)), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "calls_per_sample": inner, "samples": samples}


def host_baseline(m, classes):
    """seconds per batch of the scipy path of each op on the bands input, the upload of the fp32 result included"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    import dt_ref

    def edt_batch(site_sets):                                # [planes][images] -> fp32 (images, planes, h, w) on the device
        t0 = time.perf_counter()
        out = np.stack([np.stack([ndimage.distance_transform_edt(~s) if s.any() else np.full(s.shape, np.inf) for s in plane])
                        for plane in site_sets], axis=1).astype(np.float32)
        t1 = time.perf_counter()
        torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        return {"edt_s": round(t1 - t0, 3), "upload_s": round(time.perf_counter() - t1, 4), "edt_calls": len(site_sets) * len(site_sets[0])}

    boundary = [list(dt_ref.sites(m, classes, "boundary"))]
    cls = [list(dt_ref.sites(m, classes, ("class", c))) for c in range(classes)]
    other = [list(dt_ref.sites(m, classes, ("other", c))) for c in range(classes)]
    res = {"threads": "scipy's edt runs on one thread", "boundary": edt_batch(boundary), "classes9": edt_batch(cls)}
    res["weight"] = res["boundary"]                          # the profile of the distance is one more numpy pass: not timed
    o = edt_batch(other)
    res["signed9"] = {"edt_s": round(res["classes9"]["edt_s"] + o["edt_s"], 3), "upload_s": o["upload_s"],
                      "edt_calls": res["classes9"]["edt_calls"] + o["edt_calls"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--min-sample-ms", type=float, default=50.0)
    ap.add_argument("--inputs", default="bands6,noise3,corner")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--dtypes", default="uint8,int64")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy baseline")
    ap.add_argument("--step-ms", type=float, default=25.561,
                    help="the cfg2 training step the weight map is added to (profiles/r05_ab_bench.jsonl, tree 'change')")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distance_bench needs a GPU: a time taken anywhere else says nothing")
    from retinal_oct_image_segmentation_via_deep_learning_amd import distance

    shape = (a.images, a.height, a.width)
    npix = a.images * a.height * a.width
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy = timed(lambda: dst.copy_(src), a.warmup, a.samples, a.min_sample_ms)
    copy_rate = 2 * src.numel() / (copy["ms_median"] * 1e-3)          # bytes per second, read + write
    del src, dst
    wmap = distance.DistanceWeightMap.gaussian(a.classes, 10.0, 5.0)
    class_planes = [("class", c) for c in range(a.classes)]
    res = {"shape": list(shape), "block": list(distance.block()), "classes": a.classes, "warmup": a.warmup,
           "min_sample_ms": a.min_sample_ms, "copy_256MiB": copy, "copy_rate_GBps": round(copy_rate / 1e9, 1),
           "gaussian_table_entries": int(wmap.table.numel()), "cfg2_step_ms": a.step_ms, "inputs": {}}
    for kind in a.inputs.split(","):
        m = inputs(kind, shape, np.random.default_rng(0))
        entry = {}
        for dtype in a.dtypes.split(","):
            x = torch.from_numpy(m).to(getattr(torch, dtype)).cuda()
            calls = {"weight": lambda: wmap(x),
                     "boundary": lambda: distance.squared_distance(x, a.classes, ["boundary"]),
                     "classes9": lambda: distance.squared_distance(x, a.classes, class_planes),
                     "signed9": lambda: distance.signed_distance(x, a.classes)}
            for op in a.ops.split(","):
                r = timed(calls[op], a.warmup, a.samples, a.min_sample_ms)
                r["bytes_per_pixel"] = bytes_per_pixel(op, dtype, a.classes)
                r["floor_ms"] = round(r["bytes_per_pixel"] * npix / copy_rate * 1e3, 4)
                r["times_floor"] = round(r["ms_median"] / r["floor_ms"], 2)
                if op == "weight":
                    r["percent_of_cfg2_step"] = round(100.0 * r["ms_median"] / a.step_ms, 2)
                entry[f"{op}_{dtype}"] = r
                print(kind, dtype, op, r, flush=True)
        d2 = distance.squared_distance(x, a.classes, ["boundary"])
        far = d2 == distance.FAR
        entry["boundary_largest_d2"] = int(d2[~far].max()) if bool((~far).any()) else None
        if kind == "corner":
            entry["class1_largest_d2"] = int(distance.squared_distance(x, a.classes, [("class", 1)]).max())
        res["inputs"][kind] = entry
    res["host_scipy_bands6"] = "skipped" if a.no_host else host_baseline(inputs("bands6", shape, np.random.default_rng(0)), a.classes)
    if res["host_scipy_bands6"] is None:
        res["host_scipy_bands6"] = "absent: scipy is not installed"
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
