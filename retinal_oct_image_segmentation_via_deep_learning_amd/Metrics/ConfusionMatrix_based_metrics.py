"""Drop-in for Metrics/ConfusionMatrix_based_metrics.py (reference :4-84): accuracy, sensitivity,
precision, specificity from ONE confusion-count kernel.  `auc_score` runs on the device where that is exact: a CUDA pair of
equal shape with bf16 / uint8 / bool scores and uint8 / bool labels goes through ONE oct_score_eval_update into a one-channel
histogram of the 16-bit score key (evaluation.ScoreEvaluator; no sort, bf16 accepted) and returns sklearn's value, ties
counted half.  Every other input -- numpy arrays, fp32 / fp16 / float64 device tensors, mixed devices -- and every edge case
(a missing class, a label above 1, a NaN score) takes the reference's host route through sklearn, so the edge-case behaviour
stays sklearn's."""
import numpy as np

from ._counts import confusion_sums


def _res(v, f32):
    return np.float32(v) if f32 else np.float64(v)


def accuracy(y_true, y_pred):
    """(TP + TN) / N, no epsilon (reference :4-18)"""
    (tp, _, _, tn, _, _), n, f32 = confusion_sums(y_true, y_pred)
    if n == 0:
        return _res(float("nan"), f32)
    return _res((tp + tn) / n, f32)


def sensitivity(y_true, y_pred):
    """TP / (TP + FN + 1e-7) (reference :20-33)"""
    (tp, _, _, _, _, fn), _, f32 = confusion_sums(y_true, y_pred)
    return _res(tp / (tp + fn + 1e-7), f32)


def precision(y_true, y_pred):
    """TP / (TP + FP + 1e-7) (reference :35-48)"""
    (tp, _, _, _, fp, _), _, f32 = confusion_sums(y_true, y_pred)
    return _res(tp / (tp + fp + 1e-7), f32)


def specificity(y_true, y_pred):
    """TN / (TN + FP + 1e-7) (reference :50-63)"""
    (_, _, _, tn, fp, _), _, f32 = confusion_sums(y_true, y_pred)
    return _res(tn / (tn + fp + 1e-7), f32)


def _auc_on_device(y_true, y_pred):
    """np.float64 AUC of a device pair whose scores are 16-bit (exact), or None where the host route has to answer"""
    import torch
    if not (torch.is_tensor(y_true) and torch.is_tensor(y_pred) and y_true.is_cuda and y_pred.is_cuda):
        return None
    if y_true.device != y_pred.device or y_true.shape != y_pred.shape or not 0 < y_true.numel() < 2 ** 31:
        return None
    if y_pred.dtype not in (torch.bfloat16, torch.uint8, torch.bool) or y_true.dtype not in (torch.uint8, torch.bool):
        return None
    from ..evaluation import ScoreEvaluator, _auc_from_state
    n = y_true.numel()
    ev = ScoreEvaluator(1, logits=False)
    ev.update(y_true.reshape(1, 1, 1, n), y_pred.reshape(1, 1, 1, n))
    auc, nan, invalid = _auc_from_state(ev._host_state())
    if auc is None or invalid > 0 or nan > 0:
        return None   # sklearn decides what a missing class, a third label or a NaN score mean
    return np.float64(auc)


def _auc_on_host(y_true, y_pred):
    """the reference's route: sklearn on flattened host copies (bf16, which numpy does not have, widened to fp32 first)"""
    from sklearn.metrics import roc_auc_score
    import torch
    if torch.is_tensor(y_pred) and y_pred.dtype == torch.bfloat16:
        y_pred = y_pred.float()
    yt = np.asarray(y_true.cpu() if hasattr(y_true, "cpu") else y_true).flatten()
    yp = np.asarray(y_pred.cpu() if hasattr(y_pred, "cpu") else y_pred).flatten()
    try:
        return roc_auc_score(yt, yp)
    except ValueError:
        return 0.0


def auc_score(y_true, y_pred):
    """Area under the ROC curve (reference :65-84): on the device where the score histogram is exact, else sklearn on the host."""
    auc = _auc_on_device(y_true, y_pred)
    return auc if auc is not None else _auc_on_host(y_true, y_pred)
