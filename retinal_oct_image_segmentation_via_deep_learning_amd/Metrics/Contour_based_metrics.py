"""Drop-in for Metrics/Contour_based_metrics.py (reference :5-73): Hausdorff distance, its 95th percentile, the average
symmetric surface distance and the mean absolute difference of two binary masks.

The reference extracts contours with skimage.find_contours(mask, 0.5) and searches the nearest contour point with an O(n^2)
Python loop.  Here the contour point set is the vertex set of marching squares at level 0.5 -- the midpoint of every in-image
pair of 4-adjacent pixels of which exactly one is in the mask -- and an exact Euclidean nearest-point search runs on the
MI355X as a 1-image, 1-class update of evaluation.BoundaryEvaluator (csrc/contour.hip); the three distances come from exact
integers (evaluation.contour_metrics_from_records).

Deviations from the reference, by decision:
  * the reference scores only the first contour find_contours returns (which one is first depends on the contour order) and
    counts the first vertex of a closed contour twice; here all contours count, each vertex once.  For one simply connected
    object off the image border hausdorff_distance is the reference's value; hausdorff_distance_95 and assd differ from it
    only by the weight of the repeated vertex;
  * a mask without a contour (empty, or filling the image) gives NaN where the reference raises IndexError;
  * skimage is not a dependency of this package: the equivalence above holds by construction and is not pinned by a test.
Integer and bool masks are read as `!= 0`, float masks as `> 0.5`; inputs are 2-D numpy arrays or torch tensors."""
import numpy as np
import torch

from ._counts import _ELEM, _prepare
from .. import _lib as L


def _mask(a, what):
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if a.dim() != 2:
        raise ValueError(f"{what} must be a 2-D mask, got shape {tuple(a.shape)}")
    return a


def _contour(y_true, y_pred):
    from ..evaluation import BoundaryEvaluator
    yt, yp = _mask(y_true, "y_true"), _mask(y_pred, "y_pred")
    if yt.shape != yp.shape:
        raise ValueError(f"y_true {tuple(yt.shape)} and y_pred {tuple(yp.shape)} must have the same shape")
    dev = yt.device if yt.is_cuda else yp.device if yp.is_cuda else torch.device("cuda")
    # class 1 = inside the mask; the kernel scores classes [0, C), so the mask itself is class 0 of a 1-class map and the
    # background (label 1) belongs to no class
    maps = [(~((a > 0.5) if a.is_floating_point() else (a != 0))).to(device=dev, dtype=torch.uint8) for a in (yt, yp)]
    return BoundaryEvaluator(1).update(maps[0], maps[1]).compute()


def hausdorff_distance(y_true, y_pred):
    """max over both directions of the largest distance from a contour point to the other contour (reference :5-22)"""
    return np.float64(_contour(y_true, y_pred)["hausdorff"][0, 0])


def hausdorff_distance_95(y_true, y_pred):
    """max over both directions of np.percentile(distances, 95) (reference :24-39)"""
    return np.float64(_contour(y_true, y_pred)["hd95"][0, 0])


def assd(y_true, y_pred):
    """mean of the two directed mean distances (reference :41-56)"""
    return np.float64(_contour(y_true, y_pred)["assd"][0, 0])


def mad(y_true, y_pred):
    """mean |y_true - y_pred|, always float64 (reference :58-73 casts both masks to float first).  The inputs go through
    PixelError_based_metrics.mean_squared_error's preparation; the sum is oct_column_absdiff_sum on a one-row view (every
    element its own column), integers exact in int64, float masks in float64 like the reference's cast."""
    yt, yp, _, kdt = _prepare(y_true, y_pred)
    n = yt.numel()
    if n == 0:
        return np.float64("nan")
    if kdt.kind == "f" and kdt != np.dtype(np.float64):
        yt, yp, kdt = yt.to(torch.float64), yp.to(torch.float64), np.dtype(np.float64)
    out = torch.empty(1, dtype=torch.float64, device=yt.device)
    L.check(L.lib().oct_column_absdiff_sum(yt.data_ptr(), yp.data_ptr(), _ELEM[kdt], 0, 1, n, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "oct_column_absdiff_sum")
    return np.float64(out.item() / n)
