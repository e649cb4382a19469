"""The remaining metrics of the reference's validation_all_metrics (unetr_segmentation_3d.py:134-209, built at :485-496),
with MONAI 0.6.0's call signatures:

    precision_metric = ConfusionMatrixMetric(include_background=True, reduction="mean", get_not_nans=False, metric_name="precision")
    hsd_metric = HausdorffDistanceMetric(include_background=True, reduction="mean", get_not_nans=False)
    hsd_metric(y_pred=[one-hot ...], y=[one-hot ...]); hsd_metric.aggregate(); precision_metric.aggregate()[0]

The Hausdorff distance is the HIP pipeline of csrc/metrics.hip (bounding boxes, edges and an exact squared Euclidean distance
transform per item and class, all on the device); the confusion matrix reuses the counting kernel behind DiceMetric
(unetr_dice_counts).  Semantics are restated in DESIGN.md section 11.  No CPU fallback.
"""
from typing import Optional, Sequence, Union

import torch

from . import functional as Fn
from ._capi import call, load
from .inference import dice_counts

# Hausdorff workspace budget for the per-(b, c) slots; a single pair always gets its slot
HD_SLOT_BUDGET_BYTES = 1 << 30
_HD_MAX_EXTENT = 512
_HD_MAX_CLASSES = 32


def _stack(v):
    return torch.stack(list(v)) if isinstance(v, (list, tuple)) else v


def do_metric_reduction(f: torch.Tensor, reduction: str) -> torch.Tensor:
    """monai.metrics.utils.do_metric_reduction (0.6.0) for "mean" and "mean_batch": NaN entries are ignored, an inf stays"""
    f = f.clone()
    nans = torch.isnan(f)
    not_nans = (~nans).to(f.dtype)
    f[nans] = 0
    zero = torch.zeros(1, device=f.device, dtype=f.dtype)
    if reduction == "mean":
        nn_c = not_nans.sum(dim=1)
        f = torch.where(nn_c > 0, f.sum(dim=1) / nn_c, zero)          # channel average
        nn_b = (nn_c > 0).to(f.dtype).sum(dim=0)
        return torch.where(nn_b > 0, f.sum(dim=0) / nn_b, zero)       # batch average
    nn_b = not_nans.sum(dim=0)
    return torch.where(nn_b > 0, f.sum(dim=0) / nn_b, zero)           # "mean_batch"


def _check_reduction(cls, reduction, get_not_nans):
    if get_not_nans or reduction not in ("mean", "mean_batch"):
        raise NotImplementedError(f"{cls}(reduction='mean'|'mean_batch', get_not_nans=False): other reductions and "
                                  f"get_not_nans=True are not implemented")


def hausdorff_distance(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = False,
                       percentile: Optional[float] = None, directed: bool = False, from_logits: bool = False) -> torch.Tensor:
    """[B, C] float64 (C - 1 columns without the background) Hausdorff distance per item and class, on the device"""
    Fn._require_gpu(y_pred)
    Fn._require_gpu(y)
    if y_pred.dim() != 5:
        raise ValueError("3-D volumes [B,C,D,H,W] expected")
    y_pred = y_pred.contiguous()
    y = y.contiguous()
    B, C, D, H, W = y_pred.shape
    if from_logits and y.numel() != B * D * H * W:
        raise ValueError("from_logits: y must hold one class id per voxel [B,1,*spatial]")
    if not from_logits and y.shape != y_pred.shape:
        raise ValueError("y_pred and y must have the same one-hot shape")
    if C > _HD_MAX_CLASSES or max(D, H, W) > _HD_MAX_EXTENT:
        raise NotImplementedError(f"HausdorffDistanceMetric: at most {_HD_MAX_CLASSES} classes and {_HD_MAX_EXTENT} voxels "
                                  f"along each axis (got C={C}, {D}x{H}x{W})")
    c0 = 0 if include_background else 1
    out = torch.empty(B, C - c0, dtype=torch.float64, device=y_pred.device)
    if C - c0 == 0:
        return out
    use_pct = int(bool(percentile))           # MONAI: `if not percentile` -> max (so percentile=0 takes the max too)
    q = float(percentile) / 100.0 if use_pct else 0.0
    lib = load()
    npairs = B * (C - c0)
    base = lib.unetr_hausdorff_workspace_bytes(B, C, D, H, W, 0, use_pct)
    per_pair = lib.unetr_hausdorff_workspace_bytes(B, C, D, H, W, 1, use_pct) - base
    group = max(1, min(npairs, HD_SLOT_BUDGET_BYTES // per_pair))
    ws = torch.empty(lib.unetr_hausdorff_workspace_bytes(B, C, D, H, W, group, use_pct), dtype=torch.uint8,
                     device=y_pred.device)
    call("unetr_hausdorff", y_pred.data_ptr(), y.data_ptr(), B, C, D, H, W, c0, int(from_logits), use_pct, q, int(directed),
         out.data_ptr(), ws.data_ptr(), ws.numel(), group, Fn._stream())
    return out


class HausdorffDistanceMetric:
    """monai.metrics.HausdorffDistanceMetric (0.6.0), euclidean distance in voxel units.  ``__call__`` takes batched one-hot
    tensors or lists of per-item tensors (decollate_batch + AsDiscrete at unetr_segmentation_3d.py:144-151) and buffers the
    per-item, per-class distances ([B, C] float64; NaN where neither mask has an edge, inf where only one does);
    ``from_logits`` fuses argmax + one-hot (y then holds class ids [B,1,D,H,W]) into the first kernel."""

    def __init__(self, include_background: bool = False, distance_metric: str = "euclidean", percentile: Optional[float] = None,
                 directed: bool = False, reduction: str = "mean", get_not_nans: bool = False):
        if distance_metric != "euclidean":
            raise NotImplementedError(f"distance_metric={distance_metric!r}: only 'euclidean' is implemented")
        _check_reduction("HausdorffDistanceMetric", reduction, get_not_nans)
        if percentile is not None and not 0 <= percentile <= 100:
            raise ValueError(f"percentile should be a value between 0 and 100, get {percentile}.")
        self.include_background = include_background
        self.percentile = percentile
        self.directed = directed
        self.reduction = reduction
        self._buf = []

    def __call__(self, y_pred, y, from_logits: bool = False):
        f = hausdorff_distance(_stack(y_pred), _stack(y), self.include_background, self.percentile, self.directed, from_logits)
        self._buf.append(f)
        return f

    def aggregate(self):
        return do_metric_reduction(torch.cat(self._buf), self.reduction)

    def reset(self):
        self._buf = []


# monai.metrics.confusion_matrix.check_confusion_matrix_metric_name (0.6.0), restricted to the ratios below
_CM_NAMES = {
    "tpr": ("sensitivity", "recall", "hit_rate", "true_positive_rate", "tpr"),
    "tnr": ("specificity", "selectivity", "true_negative_rate", "tnr"),
    "ppv": ("precision", "positive_predictive_value", "ppv"),
    "npv": ("negative_predictive_value", "npv"),
    "fnr": ("miss_rate", "false_negative_rate", "fnr"),
    "fpr": ("fall_out", "false_positive_rate", "fpr"),
    "fdr": ("false_discovery_rate", "fdr"),
    "for": ("false_omission_rate", "for"),
    "ts": ("threat_score", "critical_success_index", "ts", "csi"),
    "acc": ("accuracy", "acc"),
    "f1": ("f1_score", "f1"),
}
_CM_ALIAS = {alias: key for key, names in _CM_NAMES.items() for alias in names}


def confusion_metric_key(metric_name: str) -> str:
    key = _CM_ALIAS.get(metric_name.replace(" ", "_").lower())
    if key is None:
        names = ", ".join(n for names in _CM_NAMES.values() for n in names)
        raise NotImplementedError(f"confusion matrix metric {metric_name!r} is not implemented; supported: {names}")
    return key


def compute_confusion_matrix_metric(metric_name: str, cm: torch.Tensor) -> torch.Tensor:
    """monai.metrics.compute_confusion_matrix_metric (0.6.0): ratio of the counts [..., 4] = (tp, fp, tn, fn); NaN where the
    denominator is 0.  Counts [4] (reduced by "mean") give a one-element tensor, as in MONAI."""
    key = confusion_metric_key(metric_name)
    if cm.dim() == 1:
        cm = cm.unsqueeze(0)
    tp, fp, tn, fn = cm[..., 0], cm[..., 1], cm[..., 2], cm[..., 3]
    p, n = tp + fn, fp + tn
    num, den = {
        "tpr": (tp, p), "tnr": (tn, n), "ppv": (tp, tp + fp), "npv": (tn, tn + fn), "fnr": (fn, p), "fpr": (fp, n),
        "fdr": (fp, fp + tp), "for": (fn, fn + tn), "ts": (tp, tp + fn + fp), "acc": (tp + tn, p + n),
        "f1": (tp * 2.0, tp * 2.0 + fn + fp),
    }[key]
    nan = torch.tensor(float("nan"), device=cm.device, dtype=cm.dtype)
    return torch.where(den != 0, num / den, nan)


def confusion_matrix(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = True,
                     from_logits: bool = False) -> torch.Tensor:
    """[B, C, 4] float64 (tp, fp, tn, fn) per item and class from the Dice counting kernel (C <= 16)"""
    Fn._require_gpu(y_pred)
    c = dice_counts(y_pred, y, from_logits)
    V = y_pred[0, 0].numel()
    tp = c[..., 0]
    fp = c[..., 1] - tp
    fn = c[..., 2] - tp
    tn = V - tp - fp - fn
    cm = torch.stack([tp, fp, tn, fn], dim=-1)
    return cm if include_background else cm[:, 1:]


class ConfusionMatrixMetric:
    """monai.metrics.ConfusionMatrixMetric (0.6.0) for binarised (one-hot) inputs, as the reference's precision / recall
    instances (unetr_segmentation_3d.py:487-494).  ``__call__`` buffers [B, C, 4] float64 counts (tp, fp, tn, fn);
    ``aggregate()`` returns a list with one entry per metric name.  At most 16 classes (the counting kernel's limit)."""

    def __init__(self, include_background: bool = True, metric_name: Union[Sequence[str], str] = "hit_rate",
                 compute_sample: bool = False, reduction: str = "mean", get_not_nans: bool = False):
        _check_reduction("ConfusionMatrixMetric", reduction, get_not_nans)
        self.metric_name = (metric_name,) if isinstance(metric_name, str) else tuple(metric_name)
        for name in self.metric_name:
            confusion_metric_key(name)
        self.include_background = include_background
        self.compute_sample = compute_sample
        self.reduction = reduction
        self._buf = []

    def __call__(self, y_pred, y, from_logits: bool = False):
        cm = confusion_matrix(_stack(y_pred), _stack(y), self.include_background, from_logits)
        self._buf.append(cm)
        return cm

    def aggregate(self):
        data = torch.cat(self._buf)
        results = []
        for name in self.metric_name:
            if self.compute_sample:
                results.append(do_metric_reduction(compute_confusion_matrix_metric(name, data), self.reduction))
            else:
                results.append(compute_confusion_matrix_metric(name, do_metric_reduction(data, self.reduction)))
        return results

    def reset(self):
        self._buf = []
