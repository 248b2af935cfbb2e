"""Time of one BoundaryEvaluator.update on the MI355X: 32 x 512 x 1024 layered 9-class uint8 maps (tests/eval_ref.layered_maps),
HIP events around one update, 5 warm-up runs, median of 20.  Prints one JSON line with the milliseconds per update, the
workspace bytes in use and the number of kernel chunks.

    python tools/contour_bench.py [--images 32] [--height 512] [--width 1024] [--classes 9] [--max-workspace-bytes N]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=9)
    ap.add_argument("--max-workspace-bytes", type=int, default=256 << 20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contour_bench needs a GPU: a time taken anywhere else says nothing")
    import eval_ref
    from retinal_oct_image_segmentation_via_deep_learning_amd import evaluation

    shape = (a.images, a.height, a.width)
    t, p = eval_ref.layered_maps(np.random.default_rng(0), shape, a.classes)
    dt, dp = torch.from_numpy(t).to(torch.uint8).cuda(), torch.from_numpy(p).to(torch.uint8).cuda()
    ev = evaluation.BoundaryEvaluator(a.classes, max_workspace_bytes=a.max_workspace_bytes)
    for _ in range(a.warmup):
        ev.reset().update(dt, dp)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.runs):
        ev.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ev.update(dt, dp)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    m = ev.compute()
    import ctypes as C
    from retinal_oct_image_segmentation_via_deep_learning_amd import _lib as L
    one = L.lib().oct_contour_workspace_bytes(C.byref(L.ContourDesc(1, a.height, a.width, a.classes, 0, 0, 0, 0)))
    per_chunk = min(a.images, a.max_workspace_bytes // one)
    print(json.dumps({
        "shape": list(shape), "classes": a.classes, "dtype": "uint8",
        "ms_per_update_median": round(float(np.median(times)), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
        "runs": a.runs, "warmup": a.warmup, "workspace_bytes": int(ev._workspace.numel()), "workspace_bytes_per_image": int(one),
        "max_workspace_bytes": a.max_workspace_bytes, "images_per_chunk": per_chunk, "chunks": -(-a.images // per_chunk),
        "defined": int(m["defined"].sum()), "records": int(m["defined"].size),
        "mean_hd95": [round(float(v), 4) for v in m["mean_hd95"]],
    }))


if __name__ == "__main__":
    main()
