"""Times of the connected-component entry points on the MI355X for the cfg2 validation batch, 32 x 512 x 1024 nine-class uint8:
labelling (postprocess.connected_components), labelling + filter (ComponentFilter with every rule on) and one
LesionEvaluator.update, on two inputs -- "layers": retinal-layer bands (tests/eval_ref.layered_maps) with a few hundred small
blobs of the last class, and "noise3": uniform 3-class noise, the hard case (a component per two or three pixels).  HIP events
around each call, warm-up runs, median.  Next to each time stands the floor: the bytes the launch sequence must move divided
by a device copy rate measured in the same run (a 256 MiB copy, read + write counted).

Bytes per pixel of the sequences as they are launched, N pixels, uint8 maps:
  label    local 1 (map) + 1 (class bytes) + 4 (parents) + 4 (areas) written; flatten 4 + 4 read               = 18
  filter   label + largest-component pass 4 (areas) + apply 1 (map) + 4 (roots) + 1 (out)                       = 28
  lesion   two labels (the prediction's also reads the target: + 1) + 8 cleared + overlap pass 2 + 8
           + count pass 2 + 16                                                                                  = 73
The gathers at the roots (areas in the apply pass, parents in the flatten pass) and the border pass are not counted.

    python tools/components_bench.py [--out profiles/components_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES_PER_PIXEL = {"label": 18, "filter": 28, "lesion": 73}


def inputs(kind, shape, classes, rng):
    import eval_ref
    if kind == "noise3":
        t, p = eval_ref.random_maps(rng, shape, 3)
        return t, p
    t, p = eval_ref.layered_maps(rng, shape, classes)
    t, p = t.copy(), p.copy()
    n, h, w = shape
    for b in range(n):                                   # ten blobs per image: 320 in the batch, radius 2..6
        for _ in range(10):
            cy, cx, r = rng.integers(8, h - 8), rng.integers(8, w - 8), rng.integers(2, 7)
            yy, xx = np.ogrid[-r:r + 1, -r:r + 1]
            disc = yy * yy + xx * xx <= r * r
            for m, dy in ((t, 0), (p, int(rng.integers(-2, 3)))):
                view = m[b, cy - r + dy:cy + r + 1 + dy, cx - r:cx + r + 1]
                view[disc[:view.shape[0]]] = classes - 1
    return t, p


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"ms_median": round(float(np.median(times)), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs a GPU: a time taken anywhere else says nothing")
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation, postprocess

    shape = (a.images, a.height, a.width)
    npix = a.images * a.height * a.width
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy = timed(lambda: dst.copy_(src), a.warmup, a.runs)
    copy_rate = 2 * src.numel() / (copy["ms_median"] * 1e-3)          # bytes per second, read + write
    del src, dst
    res = {"shape": list(shape), "dtype": "uint8", "tile": list(postprocess.tile()), "runs": a.runs, "warmup": a.warmup,
           "copy_256MiB": copy, "copy_rate_GBps": round(copy_rate / 1e9, 1), "bytes_per_pixel": BYTES_PER_PIXEL, "inputs": {}}
    for kind in ("layers", "noise3"):
        classes = 3 if kind == "noise3" else a.classes
        t, p = inputs(kind, shape, a.classes, np.random.default_rng(0))
        dt, dp = torch.from_numpy(t).to(torch.uint8).cuda(), torch.from_numpy(p).to(torch.uint8).cuda()
        entry = {"classes": classes}
        for conn in (4, 8):
            flt = postprocess.ComponentFilter(classes, min_area=8, keep_largest=[1] * (classes - 1) + [0], fill_enclosed=1,
                                              connectivity=conn)
            ev = evaluation.LesionEvaluator(classes, conn, max_workspace_bytes=1 << 30)
            calls = {"label": lambda: postprocess.connected_components(dp, classes, conn),
                     "filter": lambda: flt(dp),
                     "lesion": lambda: ev.update(dt, dp)}
            for name, fn in calls.items():
                r = timed(fn, a.warmup, a.runs)
                r["floor_ms"] = round(BYTES_PER_PIXEL[name] * npix / copy_rate * 1e3, 3)
                r["times_floor"] = round(r["ms_median"] / r["floor_ms"], 2)
                entry[f"{name}_c{conn}"] = r
            _, info = postprocess.connected_components(dp, classes, conn)
            entry[f"components_c{conn}"] = int((info != 0).sum())
            m = ev.compute()
            entry[f"lesion_c{conn}_sensitivity_last_class"] = float(m["sensitivity"][classes - 1])
        res["inputs"][kind] = entry
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
