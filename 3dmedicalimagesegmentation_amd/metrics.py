"""The remaining metrics of the reference's validation_all_metrics (unetr_segmentation_3d.py:134-209, built at :485-496),
with MONAI 0.6.0's call signatures:

    precision_metric = ConfusionMatrixMetric(include_background=True, reduction="mean", get_not_nans=False, metric_name="precision")
    hsd_metric = HausdorffDistanceMetric(include_background=True, reduction="mean", get_not_nans=False)
    hsd_metric(y_pred=[one-hot ...], y=[one-hot ...]); hsd_metric.aggregate(); precision_metric.aggregate()[0]

The Hausdorff distance is the HIP pipeline of csrc/metrics.hip (bounding boxes, edges and an exact squared Euclidean distance
transform per item and class, all on the device); the confusion matrix reuses the counting kernel behind DiceMetric
(unetr_dice_counts).  Semantics are restated in DESIGN.md section 11.  No CPU fallback.

``surface_metrics`` runs the same pipeline once in float64 millimetres (``spacing``) and returns everything that is a reduction of
the two directed edge-to-edge distance fields; ``HausdorffDistanceMetric(spacing=...)``, ``SurfaceDistanceMetric`` and
``SurfaceDiceMetric`` are thin classes over it.
"""
import ctypes
import math
from typing import List, NamedTuple, Optional, Sequence, Union

import torch

from . import functional as Fn
from ._capi import call, load
from .inference import dice_counts

# Hausdorff workspace budget for the per-(b, c) slots; a single pair always gets its slot
HD_SLOT_BUDGET_BYTES = 1 << 30
_HD_MAX_EXTENT = 512
_HD_MAX_CLASSES = 32
_SM_MAX_PERCENTILES = 8


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


def _slot_group(workspace_bytes, npairs):
    """(slots processed together, workspace bytes): as many (b, c) pairs as fit HD_SLOT_BUDGET_BYTES, at least one"""
    base = workspace_bytes(0)
    group = max(1, min(npairs, HD_SLOT_BUDGET_BYTES // (workspace_bytes(1) - base)))
    return group, workspace_bytes(group)


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
    group, nbytes = _slot_group(lambda g: lib.unetr_hausdorff_workspace_bytes(B, C, D, H, W, g, use_pct), B * (C - c0))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=y_pred.device)
    call("unetr_hausdorff", y_pred.data_ptr(), y.data_ptr(), B, C, D, H, W, c0, int(from_logits), use_pct, q, int(directed),
         out.data_ptr(), ws.data_ptr(), ws.numel(), group, Fn._stream())
    return out


class SurfaceMetrics(NamedTuple):
    """what ``surface_metrics`` returns: [B, C'] float64 device tensors per field (``pct_*``: one per requested percentile)"""
    n_pred: torch.Tensor                  # edge voxels of the prediction / of the ground truth
    n_gt: torch.Tensor
    max_pg: torch.Tensor                  # max, mean of d(pred edge -> nearest gt edge) and the other way round
    max_gp: torch.Tensor
    mean_pg: torch.Tensor
    mean_gp: torch.Tensor
    pct_pg: List[torch.Tensor]
    pct_gp: List[torch.Tensor]
    within_pg: Optional[torch.Tensor]     # number of pred (gt) edges with d <= the class's threshold; None without thresholds
    within_gp: Optional[torch.Tensor]


def _check_spacing(spacing):
    if spacing is None:
        return (1.0, 1.0, 1.0)
    s = tuple(float(v) for v in spacing)
    if len(s) != 3:
        raise ValueError(f"spacing must hold three numbers (per step along D, H, W), got {spacing!r}")
    if not all(math.isfinite(v) and v > 0 for v in s):
        raise ValueError(f"spacing must be positive and finite, got {spacing!r}")
    return s


def _check_percentiles(percentiles):
    q = tuple(float(v) for v in percentiles)
    if len(q) > _SM_MAX_PERCENTILES:
        raise NotImplementedError(f"at most {_SM_MAX_PERCENTILES} percentiles per call, got {len(q)}")
    for v in q:
        if not 0 <= v <= 100:
            raise ValueError(f"percentile should be a value between 0 and 100, get {v}.")
    return q


def surface_metrics(y_pred: torch.Tensor, y: torch.Tensor, *, spacing: Optional[Sequence[float]] = None,
                    include_background: bool = False, percentiles: Sequence[float] = (),
                    thresholds: Optional[Sequence[float]] = None, from_logits: bool = False,
                    class_ids: Optional[int] = None) -> SurfaceMetrics:
    """Every surface metric of a batch from one exact distance transform in the units of ``spacing`` (per step along D, H, W;
    None = (1, 1, 1)), one ``unetr_surface_metrics`` call.  Inputs as ``hausdorff_distance`` (one-hot, or ``from_logits``), or
    with ``class_ids=C`` two uint8 class-id maps [B,1,D,H,W] of C classes (``restore_native(..., post="argmax")``, label files).
    ``percentiles`` (at most 8, each in [0, 100]) follow np.percentile's linear rule -- 0 is the minimum here; the metric
    classes apply MONAI's "falsy percentile = max".  ``thresholds``: one tolerance per evaluated class.  A direction without
    query edges is nan in max / mean / percentile; with query edges but an empty other set it is inf / inf / nan."""
    sp = _check_spacing(spacing)
    q = _check_percentiles(percentiles)
    Fn._require_gpu(y_pred, ids=class_ids is not None)
    Fn._require_gpu(y, ids=class_ids is not None)
    if y_pred.dim() != 5:
        raise ValueError("3-D volumes [B,C,D,H,W] expected")
    y_pred = y_pred.contiguous()
    y = y.contiguous()
    if class_ids is not None:
        if from_logits:
            raise ValueError("class_ids and from_logits exclude each other")
        if y_pred.dtype != torch.uint8 or y.dtype != torch.uint8 or y_pred.shape[1] != 1 or y.shape != y_pred.shape:
            raise ValueError("class_ids: y_pred and y must both be uint8 class-id maps [B,1,D,H,W]")
        B, _, D, H, W = y_pred.shape
        C, form = int(class_ids), 2
    else:
        if y_pred.dtype != torch.float32 or y.dtype != torch.float32:
            raise ValueError("float32 inputs expected (uint8 class-id maps take class_ids=C)")
        B, C, D, H, W = y_pred.shape
        form = int(bool(from_logits))
        if from_logits and y.numel() != B * D * H * W:
            raise ValueError("from_logits: y must hold one class id per voxel [B,1,*spatial]")
        if not from_logits and y.shape != y_pred.shape:
            raise ValueError("y_pred and y must have the same one-hot shape")
    if not 0 < C <= _HD_MAX_CLASSES or max(D, H, W) > _HD_MAX_EXTENT:
        raise NotImplementedError(f"surface_metrics: at most {_HD_MAX_CLASSES} classes and {_HD_MAX_EXTENT} voxels along each "
                                  f"axis (got C={C}, {D}x{H}x{W})")
    c0 = 0 if include_background else 1
    Cp = C - c0
    tau = None
    if thresholds is not None:
        tau = tuple(float(v) for v in thresholds)
        if len(tau) != Cp:
            raise ValueError(f"one threshold per evaluated class expected ({Cp}), got {len(tau)}")
        if not all(v >= 0 for v in tau):
            raise ValueError(f"thresholds must be non-negative numbers, got {thresholds!r}")
    nq = len(q)
    out = torch.empty(8 + 2 * nq, B, Cp, dtype=torch.float64, device=y_pred.device)
    if Cp > 0:
        lib = load()
        group, nbytes = _slot_group(lambda g: lib.unetr_surface_metrics_workspace_bytes(B, C, D, H, W, g, nq), B * Cp)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=y_pred.device)
        call("unetr_surface_metrics", y_pred.data_ptr(), y.data_ptr(), B, C, D, H, W, c0, form, (ctypes.c_double * 3)(*sp),
             (ctypes.c_double * nq)(*[v / 100.0 for v in q]) if nq else None, nq,
             (ctypes.c_double * Cp)(*tau) if tau is not None else None, out.data_ptr(), ws.data_ptr(), ws.numel(), group,
             Fn._stream())
    return SurfaceMetrics(out[0], out[1], out[2], out[3], out[4], out[5], [out[8 + k] for k in range(nq)],
                          [out[8 + nq + k] for k in range(nq)], out[6] if tau is not None else None,
                          out[7] if tau is not None else None)


class _SurfaceMetric:
    """the __call__ / aggregate / reset protocol of the metrics over ``surface_metrics``; a subclass gives ``_request`` (the
    keywords of the call) and ``_score`` (record -> [B, C'])"""

    def _init(self, include_background, distance_metric, reduction, get_not_nans, spacing):
        if distance_metric != "euclidean":
            raise NotImplementedError(f"distance_metric={distance_metric!r}: only 'euclidean' is implemented")
        _check_reduction(type(self).__name__, reduction, get_not_nans)
        self.include_background = include_background
        self.reduction = reduction
        self.spacing = None if spacing is None else _check_spacing(spacing)
        self._buf = []

    def __call__(self, y_pred, y, from_logits: bool = False, spacing: Optional[Sequence[float]] = None,
                 class_ids: Optional[int] = None):
        f = self._measure(_stack(y_pred), _stack(y), from_logits, self.spacing if spacing is None else spacing, class_ids)
        self._buf.append(f)
        return f

    def _measure(self, y_pred, y, from_logits, spacing, class_ids):
        return self._score(surface_metrics(y_pred, y, spacing=spacing, include_background=self.include_background,
                                           from_logits=from_logits, class_ids=class_ids, **self._request()))

    def aggregate(self):
        return do_metric_reduction(torch.cat(self._buf), self.reduction)

    def reset(self):
        self._buf = []


class HausdorffDistanceMetric(_SurfaceMetric):
    """monai.metrics.HausdorffDistanceMetric (0.6.0), euclidean distance.  ``__call__`` takes batched one-hot
    tensors or lists of per-item tensors (decollate_batch + AsDiscrete at unetr_segmentation_3d.py:144-151) and buffers the
    per-item, per-class distances ([B, C] float64; NaN where neither mask has an edge, inf where only one does);
    ``from_logits`` fuses argmax + one-hot (y then holds class ids [B,1,D,H,W]) into the first kernel.  Without a ``spacing``
    (here or per call) distances are in voxel units on the integer pipeline (unetr_hausdorff); with one they are in its units
    (millimetres) through ``surface_metrics``, with the same nan / inf / percentile / directed / max rules."""

    def __init__(self, include_background: bool = False, distance_metric: str = "euclidean", percentile: Optional[float] = None,
                 directed: bool = False, reduction: str = "mean", get_not_nans: bool = False,
                 spacing: Optional[Sequence[float]] = None):
        self._init(include_background, distance_metric, reduction, get_not_nans, spacing)
        if percentile is not None and not 0 <= percentile <= 100:
            raise ValueError(f"percentile should be a value between 0 and 100, get {percentile}.")
        self.percentile = percentile
        self.directed = directed

    def _measure(self, y_pred, y, from_logits, spacing, class_ids):
        if spacing is None and class_ids is None:
            return hausdorff_distance(y_pred, y, self.include_background, self.percentile, self.directed, from_logits)
        return super()._measure(y_pred, y, from_logits, spacing, class_ids)

    def _request(self):
        return dict(percentiles=(self.percentile,)) if self.percentile else {}    # MONAI: `if not percentile` -> max

    def _score(self, r):
        d1, d2 = (r.pct_pg[0], r.pct_gp[0]) if self.percentile else (r.max_pg, r.max_gp)
        return d1.clone() if self.directed else torch.where(d2 > d1, d2, d1)       # Python max(d1, d2): d1 unless d2 > d1


class SurfaceDistanceMetric(_SurfaceMetric):
    """monai.metrics.SurfaceDistanceMetric (0.6.0), euclidean: the average distance of the prediction's edge voxels to the
    nearest edge voxel of the ground truth (nan without prediction edges, inf when only the ground truth has none);
    ``symmetric`` averages it with the same quantity the other way round (np.mean of the two)."""

    def __init__(self, include_background: bool = False, symmetric: bool = False, distance_metric: str = "euclidean",
                 reduction: str = "mean", get_not_nans: bool = False, spacing: Optional[Sequence[float]] = None):
        self._init(include_background, distance_metric, reduction, get_not_nans, spacing)
        self.symmetric = symmetric

    def _request(self):
        return {}

    def _score(self, r):
        return (r.mean_pg + r.mean_gp) / 2 if self.symmetric else r.mean_pg.clone()


class SurfaceDiceMetric(_SurfaceMetric):
    """Normalised surface Dice at one tolerance per evaluated class (the Medical Segmentation Decathlon's second metric):
    (#pred edges within tau of the gt surface + #gt edges within tau of the pred surface) / (#pred edges + #gt edges); nan when
    neither mask has an edge."""

    def __init__(self, class_thresholds: Sequence[float], include_background: bool = False, distance_metric: str = "euclidean",
                 reduction: str = "mean", get_not_nans: bool = False, spacing: Optional[Sequence[float]] = None):
        self._init(include_background, distance_metric, reduction, get_not_nans, spacing)
        self.class_thresholds = tuple(float(v) for v in class_thresholds)
        if not all(math.isfinite(v) and v >= 0 for v in self.class_thresholds):
            raise ValueError(f"class_thresholds must be non-negative and finite, got {class_thresholds!r}")

    def _request(self):
        return dict(thresholds=self.class_thresholds)

    def _score(self, r):
        return (r.within_pg + r.within_gp) / (r.n_pred + r.n_gt)


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
