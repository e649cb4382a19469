"""Instance-level segmentation metrics on the device: how many lesions were found, how well each one was segmented and how many
detections were spurious.

    r = lesion_wise_metrics(y_pred, y)                         # BraTS-2023-style lesion-wise Dice, lesion-level P / R / F1
    metric = LesionWiseMetric(metric_name="f1"); metric(y_pred=[...], y=[...]); metric.aggregate()
    q = panoptic_quality(y_pred, y)                            # tp / fp / fn, SQ, RQ, PQ at IoU > 0.5

Both are reductions of one primitive, the sparse contingency table of two canonical label maps (``label_overlaps``; the kernels
of csrc/lesion.hip, unetr_label_overlaps).  The label maps come from ``connected_components`` and, for the lesion-wise metrics,
``binary_dilation``: one dilation and one labelling of the whole ground truth replace the per-lesion loop of the definition.
Stream-ordered launches, no host synchronisation: a call can sit inside a captured graph.  Semantics are restated in DESIGN.md
section 24.  No CPU fallback.
"""
from typing import NamedTuple, Optional

import torch

from . import functional as Fn
from ._capi import call, load
from .metrics import _check_reduction, _stack, do_metric_reduction
from .morphology import _check_connectivity, binary_dilation
from .postprocess import _connectivity, connected_components

# workspace budget for the planes whose tables are built together; a single plane always gets its slot
LESION_PLANE_BUDGET_BYTES = 1 << 30
LO_FIELDS = 8                    # = UNETR_LO_FIELDS
_MAX_PAIRS = 1 << 24
_INT_MAX = 2 ** 31 - 1
_LESION, _PANOPTIC = 0, 1


class LesionWiseMetrics(NamedTuple):
    """what ``lesion_wise_metrics`` returns: [B, C'] device tensors, counts int64, the rest float64.  A plane whose pair table
    overflowed has ``overflow`` 1, NaN in every float field and -1 in ``n_tp`` / ``n_fn`` / ``n_fp``."""
    n_gt: torch.Tensor            # ground-truth lesions, the ignored ones included
    n_tp: torch.Tensor            # lesions (not ignored) with at least one matched predicted component
    n_fn: torch.Tensor            # lesions (not ignored) without one
    n_fp: torch.Tensor            # predicted components that match no lesion at all
    n_pred: torch.Tensor          # predicted components
    dice_sum: torch.Tensor        # sum of the per-lesion Dice over the lesions that are not ignored
    lesion_dice: torch.Tensor     # dice_sum / (n_tp + n_fn + n_fp); 1 when that is 0 / 0
    precision: torch.Tensor
    recall: torch.Tensor
    f1: torch.Tensor
    overflow: torch.Tensor


class PanopticQuality(NamedTuple):
    """what ``panoptic_quality`` returns: [B, C'] device tensors, counts int64, the rest float64"""
    tp: torch.Tensor
    fp: torch.Tensor
    fn: torch.Tensor
    sq: torch.Tensor
    rq: torch.Tensor
    pq: torch.Tensor
    overflow: torch.Tensor


def table_slots(max_pairs: int) -> int:
    """slots of a plane's pair table: 2 * max_pairs rounded up to a power of two"""
    s = 2
    while s < 2 * max_pairs:
        s <<= 1
    return s


def _check_max_pairs(max_pairs):
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, int) or max_pairs < 1:
        raise ValueError(f"max_pairs should be an integer >= 1, got {max_pairs!r}")
    if max_pairs > _MAX_PAIRS:
        raise NotImplementedError(f"max_pairs: at most {_MAX_PAIRS} pairs per plane, got {max_pairs}")
    return max_pairs


def label_overlaps(a: torch.Tensor, b: torch.Tensor, mask: Optional[torch.Tensor] = None, *, mode: int = _LESION,
                   min_size: int = 0, max_pairs: int = 65536, return_workspace: bool = False):
    """One ``unetr_label_overlaps`` call on two int32 canonical label maps [..., D, H, W] of equal shape (``mask``: float32 of the
    same shape or None).  Returns (counts int64 [P, 8], values float64 [P, 8]) as include/unetr_hip.h lays them out, P = the
    product of the leading dimensions; with ``return_workspace`` also the uint8 workspace, which begins with the pair tables."""
    _check_max_pairs(max_pairs)
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dim() < 4 or a.shape != b.shape:
        raise ValueError("two label maps [..., D, H, W] of the same shape expected")
    if a.dtype != torch.int32 or b.dtype != torch.int32:
        raise ValueError(f"int32 label maps expected, got {a.dtype} and {b.dtype}")
    if mask is not None and (mask.shape != a.shape or mask.dtype != torch.float32):
        raise ValueError("mask: float32 of the label maps' shape expected")
    if a.numel() == 0:
        raise ValueError("empty input")
    for t in (a, b) + (() if mask is None else (mask,)):
        if not t.is_cuda:
            Fn._require_gpu(t)                                   # raises: there is no CPU fallback
        if t.device != a.device or t.device.index != torch.cuda.current_device():
            raise RuntimeError(f"label_overlaps: tensors must live on the current device, got {t.device}")
    D, H, W = a.shape[-3:]
    planes = a.numel() // (D * H * W)
    lib = load()
    per_plane = lib.unetr_label_overlaps_workspace_bytes(D, H, W, max_pairs, 1) - lib.unetr_label_overlaps_workspace_bytes(D, H, W, max_pairs, 0)
    if per_plane <= 0:
        raise NotImplementedError(f"label_overlaps: at most 1024 voxels along each axis and 2^31 - 2 voxels per volume (got {D}x{H}x{W})")
    group = max(1, min(planes, LESION_PLANE_BUDGET_BYTES // per_plane))
    a, b = a.contiguous(), b.contiguous()
    mask = None if mask is None else mask.contiguous()
    counts = torch.empty(planes, LO_FIELDS, dtype=torch.int64, device=a.device)
    values = torch.empty(planes, LO_FIELDS, dtype=torch.float64, device=a.device)
    ws = torch.empty(lib.unetr_label_overlaps_workspace_bytes(D, H, W, max_pairs, group), dtype=torch.uint8, device=a.device)
    call("unetr_label_overlaps", a.data_ptr(), b.data_ptr(), None if mask is None else mask.data_ptr(), planes, D, H, W, mode,
         min(int(min_size), _INT_MAX), max_pairs, counts.data_ptr(), values.data_ptr(), ws.data_ptr(), ws.numel(), group, Fn._stream())
    return (counts, values, ws) if return_workspace else (counts, values)


def _binary_planes(y_pred, y, include_background, class_ids, what):
    """(pred, gt) as float32 0 / 1 tensors [B, C', D, H, W] on the device: the evaluated channels of a one-hot / multi-label
    pair, or the classes of two uint8 class-id maps"""
    if not isinstance(y_pred, torch.Tensor) or not isinstance(y, torch.Tensor) or y_pred.dim() != 5:
        raise ValueError("3-D volumes [B,C,D,H,W] expected")
    if y.shape != y_pred.shape:
        raise ValueError(f"{what}: y_pred and y must have the same shape, got {tuple(y_pred.shape)} and {tuple(y.shape)}")
    if y_pred.numel() == 0:
        raise ValueError("empty input")
    c0 = 0 if include_background else 1
    if class_ids is not None:
        if isinstance(class_ids, bool) or not isinstance(class_ids, int) or class_ids < 1:
            raise ValueError(f"class_ids should be the number of classes, got {class_ids!r}")
        if y_pred.dtype != torch.uint8 or y.dtype != torch.uint8 or y_pred.shape[1] != 1:
            raise ValueError("class_ids: y_pred and y must both be uint8 class-id maps [B,1,D,H,W]")
        Fn._require_gpu(y_pred, ids=True)
        Fn._require_gpu(y, ids=True)
        ids = torch.arange(c0, class_ids, dtype=torch.uint8, device=y.device).view(1, -1, 1, 1, 1)
        return (y_pred == ids).to(torch.float32), (y == ids).to(torch.float32)
    if y_pred.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("float32 inputs expected (uint8 class-id maps take class_ids=C)")
    Fn._require_gpu(y_pred)
    Fn._require_gpu(y)
    return (y_pred[:, c0:] != 0).to(torch.float32), (y[:, c0:] != 0).to(torch.float32)


def _check_lesion_args(dilation, dilation_connectivity, connectivity, min_lesion_voxels, max_pairs):
    if isinstance(dilation, bool) or not isinstance(dilation, int) or dilation < 0:
        raise ValueError(f"dilation should be an integer >= 0, got {dilation!r}")
    _check_connectivity(dilation_connectivity)
    _connectivity(connectivity)
    if isinstance(min_lesion_voxels, bool) or not isinstance(min_lesion_voxels, int) or min_lesion_voxels < 0:
        raise ValueError(f"min_lesion_voxels should be a non-negative integer, got {min_lesion_voxels!r}")
    _check_max_pairs(max_pairs)


def lesion_wise_metrics(y_pred: torch.Tensor, y: torch.Tensor, *, include_background: bool = False, dilation: int = 3,
                        dilation_connectivity: int = 2, connectivity: Optional[int] = None, min_lesion_voxels: int = 0,
                        max_pairs: int = 65536, class_ids: Optional[int] = None) -> LesionWiseMetrics:
    """Lesion-wise Dice and lesion-level detection scores per (item, evaluated channel).  Ground-truth components whose
    ``dilation``-step dilations (structuring element of ``dilation_connectivity``) touch are one lesion; a predicted component
    matches every lesion whose dilation it meets; the Dice of a lesion is taken against the union of its matched components;
    unmatched predicted components are false positives and add 0 terms.  Components are taken under ``connectivity`` (None = 26
    neighbours).  Lesions of fewer than ``min_lesion_voxels`` voxels are ignored together with their matches.  ``max_pairs``
    bounds the distinct (lesion, component) pairs of a plane; a plane with more is flagged in ``overflow``.  Inputs: one-hot /
    multi-label float32 [B,C,D,H,W], set where non-zero, or with ``class_ids=C`` two uint8 class-id maps [B,1,D,H,W]."""
    _check_lesion_args(dilation, dilation_connectivity, connectivity, min_lesion_voxels, max_pairs)
    pred, gt = _binary_planes(y_pred, y, include_background, class_ids, "lesion_wise_metrics")
    B, Cp = gt.shape[:2]
    if Cp == 0:
        z, f = (torch.empty(B, 0, dtype=t, device=gt.device) for t in (torch.int64, torch.float64))
        return LesionWiseMetrics(z, z, z, z, z, f, f, f, f, f, z)
    dil = binary_dilation(gt, iterations=dilation, connectivity=dilation_connectivity) if dilation else gt
    counts, values = label_overlaps(connected_components(dil, connectivity), connected_components(pred, connectivity), gt,
                                    mode=_LESION, min_size=min_lesion_voxels, max_pairs=max_pairs)
    c, v = counts.view(B, Cp, LO_FIELDS), values.view(B, Cp, LO_FIELDS)
    return LesionWiseMetrics(c[..., 0], c[..., 1], c[..., 2], c[..., 3], c[..., 4], v[..., 0], v[..., 1], v[..., 2], v[..., 3],
                             v[..., 4], c[..., 6])


def panoptic_quality(y_pred: torch.Tensor, y: torch.Tensor, *, include_background: bool = False, connectivity: Optional[int] = None,
                     max_pairs: int = 65536, class_ids: Optional[int] = None) -> PanopticQuality:
    """Panoptic quality per (item, evaluated channel) over the connected components of the two masks: a ground-truth and a
    predicted component match when their IoU exceeds 0.5 (decided in integers); sq = mean IoU of the matches (0 without one),
    rq = tp / (tp + fp / 2 + fn / 2), pq = sq * rq; a plane with no component on either side is NaN.  Inputs as
    ``lesion_wise_metrics``."""
    _connectivity(connectivity)
    _check_max_pairs(max_pairs)
    pred, gt = _binary_planes(y_pred, y, include_background, class_ids, "panoptic_quality")
    B, Cp = gt.shape[:2]
    if Cp == 0:
        z, f = (torch.empty(B, 0, dtype=t, device=gt.device) for t in (torch.int64, torch.float64))
        return PanopticQuality(z, z, z, f, f, f, z)
    counts, values = label_overlaps(connected_components(gt, connectivity), connected_components(pred, connectivity), None,
                                    mode=_PANOPTIC, max_pairs=max_pairs)
    c, v = counts.view(B, Cp, LO_FIELDS), values.view(B, Cp, LO_FIELDS)
    return PanopticQuality(c[..., 1], c[..., 3], c[..., 2], v[..., 1], v[..., 2], v[..., 3], c[..., 6])


class LesionWiseMetric:
    """One field of ``lesion_wise_metrics`` as a metric object in the shape of ``ConfusionMatrixMetric``: ``__call__(y_pred=, y=)``
    on tensors or decollated lists buffers the [B, C'] float64 values, ``aggregate()`` reduces them with ``do_metric_reduction``
    (NaN entries -- a 0 / 0, an overflowed plane -- are ignored), ``reset()`` empties the buffer."""

    _NAMES = ("lesion_dice", "f1", "precision", "recall")

    def __init__(self, metric_name: str = "lesion_dice", include_background: bool = False, reduction: str = "mean",
                 get_not_nans: bool = False, dilation: int = 3, dilation_connectivity: int = 2, connectivity: Optional[int] = None,
                 min_lesion_voxels: int = 0, max_pairs: int = 65536):
        _check_reduction("LesionWiseMetric", reduction, get_not_nans)
        if metric_name not in self._NAMES:
            raise ValueError(f"metric_name should be one of {self._NAMES}, got {metric_name!r}")
        _check_lesion_args(dilation, dilation_connectivity, connectivity, min_lesion_voxels, max_pairs)
        self.metric_name = metric_name
        self.include_background = include_background
        self.reduction = reduction
        self._kw = dict(dilation=dilation, dilation_connectivity=dilation_connectivity, connectivity=connectivity,
                        min_lesion_voxels=min_lesion_voxels, max_pairs=max_pairs)
        self._buf = []

    def __call__(self, y_pred, y, class_ids: Optional[int] = None):
        r = lesion_wise_metrics(_stack(y_pred), _stack(y), include_background=self.include_background, class_ids=class_ids, **self._kw)
        f = getattr(r, self.metric_name)
        self._buf.append(f)
        return f

    def aggregate(self):
        return do_metric_reduction(torch.cat(self._buf), self.reduction)

    def reset(self):
        self._buf = []
