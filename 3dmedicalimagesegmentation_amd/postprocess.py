"""Connected-component post-processing of a discrete prediction, on the device:

    klcc = KeepLargestConnectedComponent(applied_labels=[1], independent=True, connectivity=None)   # MONAI 0.6.0's constructor
    mask = klcc(inferer(x, net, post="argmax"))

``connected_components`` labels the 3-D components of a class-id map, a one-hot / multi-label tensor or logits;
``KeepLargestConnectedComponent`` discards every island of a class except the largest one; ``remove_small_components`` keeps
the components of at least ``min_size`` voxels.  All three are one stream-ordered call of the union-find kernels of
csrc/postprocess.hip (unetr_ccl): no host synchronisation, so they can sit inside a captured graph.  Semantics are restated in
DESIGN.md section 15.  No CPU fallback.
"""
from typing import Optional, Sequence, Union

import torch

from . import functional as Fn
from ._capi import call, load

# workspace budget for the planes labelled together; a single plane always gets its slot
CCL_PLANE_BUDGET_BYTES = 1 << 30
_CCL_MAX_EXTENT = 1024
_CCL_MAX_CLASSES = 16
_CCL_MAX_ID = 31
_INT_MAX = 2 ** 31 - 1


def _connectivity(connectivity):
    if connectivity is None:
        return 3                       # full connectivity, as skimage.measure.label
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or not 1 <= connectivity <= 3:
        raise ValueError(f"connectivity should be 1, 2, 3 or None for 3-D volumes, got {connectivity!r}")
    return connectivity


def _applied_mask(applied_labels, mode, C):
    """bit mask of the applied class ids (class-id map, logits) or channels (one-hot)"""
    if applied_labels is None:
        if mode == 0:
            return (1 << (_CCL_MAX_ID + 1)) - 2
        return (1 << C) - 1 if mode == 1 else (1 << C) - 2
    ids = [applied_labels] if isinstance(applied_labels, int) else list(applied_labels)
    if not ids:
        raise ValueError("applied_labels is empty")
    mask = 0
    for i in ids:
        if isinstance(i, bool) or int(i) != i:
            raise ValueError(f"applied_labels should hold integers, got {i!r}")
        i = int(i)
        if mode == 1:
            if not 0 <= i < C:
                raise ValueError(f"applied_labels: channel {i} is outside the {C} channels of the one-hot input")
        else:
            if i == 0:
                raise ValueError("applied_labels: 0 is the background of a class-id map and cannot be filtered")
            if i < 0 or (mode == 2 and i >= C):
                raise ValueError(f"applied_labels: class id {i} is out of range")
            if i > _CCL_MAX_ID:
                raise NotImplementedError(f"applied_labels: class ids of a class-id map go up to {_CCL_MAX_ID}, got {i}")
        mask |= 1 << i
    return mask


def _ccl(x, connectivity, applied_labels, independent, from_logits, rule=0, min_size=0, want_out=False, want_labels=False,
         want_sizes=False, want_counts=False):
    conn = _connectivity(connectivity)
    if not isinstance(x, torch.Tensor) or x.dim() != 5:
        raise ValueError("3-D volumes [B,C,D,H,W] expected")
    B, C, D, H, W = x.shape
    if x.numel() == 0:
        raise ValueError("empty input")
    if from_logits and C < 2:
        raise ValueError("from_logits: logits [B,C,D,H,W] with C >= 2 expected")
    mode = 2 if from_logits else (0 if C == 1 else 1)
    mask = _applied_mask(applied_labels, mode, C)
    if C > _CCL_MAX_CLASSES or max(D, H, W) > _CCL_MAX_EXTENT or D * H * W >= _INT_MAX:
        raise NotImplementedError(f"connected components: at most {_CCL_MAX_CLASSES} channels, {_CCL_MAX_EXTENT} voxels along "
                                  f"each axis and 2^31 - 2 voxels per volume (got C={C}, {D}x{H}x{W})")
    if x.is_cuda and x.dtype != torch.float32:
        x = x.to(torch.float32)
    Fn._require_gpu(x)
    x = x.contiguous()
    Co = C if mode == 1 else 1
    napplied = bin(mask).count("1")
    planes = B * napplied if mode == 1 and independent else B
    i32 = dict(dtype=torch.int32, device=x.device)
    # channels of a one-hot input that are not applied are not written by the kernels: they pass through / stay 0
    partial = mode == 1 and napplied < C
    out = labels = sizes = counts = None
    if want_out:
        out = x.clone() if partial else torch.empty(B, Co, D, H, W, dtype=torch.float32, device=x.device)
    elif mode == 2:
        out = torch.empty(B, 1, D, H, W, dtype=torch.float32, device=x.device)      # holds the argmax
    if want_labels:
        labels = (torch.zeros if partial else torch.empty)(B, Co, D, H, W, **i32)
    if want_sizes:
        sizes = (torch.zeros if partial else torch.empty)(B, Co, D, H, W, **i32)
    if want_counts:
        counts = torch.empty(planes, 32, **i32)
    lib = load()
    per_plane = lib.unetr_ccl_workspace_bytes(D, H, W, 1) - lib.unetr_ccl_workspace_bytes(D, H, W, 0)
    group = max(1, min(planes, CCL_PLANE_BUDGET_BYTES // per_plane))
    ws = torch.empty(lib.unetr_ccl_workspace_bytes(D, H, W, group), dtype=torch.uint8, device=x.device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    call("unetr_ccl", x.data_ptr(), ptr(out), ptr(labels), ptr(sizes), ptr(counts), B, C, D, H, W, mode, mask, int(bool(independent)),
         conn, rule, min(int(min_size), _INT_MAX), ws.data_ptr(), ws.numel(), group, Fn._stream())
    return out, labels, sizes, counts


def connected_components(x: torch.Tensor, connectivity: Optional[int] = None, applied_labels=None, independent: bool = True,
                         from_logits: bool = False, return_sizes: bool = False):
    """int32 canonical component labels of x: 1 + the smallest linear index (z*H + y)*W + x of the component's voxels, 0 for
    voxels that are not labelled.  x is a class-id map [B,1,D,H,W], a one-hot / multi-label tensor [B,C,D,H,W] (labels of the
    same shape; with ``independent=False`` every applied channel carries, where it is set, the label of the union mask) or,
    with ``from_logits``, logits [B,C,D,H,W] (labels [B,1,D,H,W] of the argmax).  ``applied_labels=None`` labels every non-zero
    id / every channel.  ``return_sizes`` adds the voxel count of each voxel's component."""
    _, labels, sizes, _ = _ccl(x, connectivity, applied_labels, independent, from_logits, want_labels=True, want_sizes=return_sizes)
    return (labels, sizes) if return_sizes else labels


def count_components(x: torch.Tensor, connectivity: Optional[int] = None, applied_labels=None, independent: bool = True,
                     from_logits: bool = False) -> torch.Tensor:
    """[planes, 32] int32 number of components per plane and class word: planes are the batch items (column = class id, or
    column 1 with ``independent=False``), or for an independent one-hot input the (item, applied channel) pairs (column 1)"""
    return _ccl(x, connectivity, applied_labels, independent, from_logits, want_counts=True)[3]


def remove_small_components(x: torch.Tensor, min_size: int, connectivity: Optional[int] = None, applied_labels=None,
                            independent: bool = True) -> torch.Tensor:
    """x with every component of fewer than ``min_size`` voxels set to 0 (skimage.morphology.remove_small_objects per class)"""
    if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 0:
        raise ValueError(f"min_size should be a non-negative integer, got {min_size!r}")
    return _ccl(x, connectivity, applied_labels, independent, False, rule=1, min_size=int(min_size), want_out=True)[0]


class KeepLargestConnectedComponent:
    """monai.transforms.KeepLargestConnectedComponent (0.6.0): per class of ``applied_labels`` keep the component with the most
    voxels (ties: the one whose first voxel comes first in raster order) and set the others to 0.  With a one-channel class-id
    map ``applied_labels`` are class ids, with a one-hot input they are channels; ``independent=False`` treats the applied
    labels as one foreground.  ``__call__`` takes [B,C,D,H,W], a decollated [C,D,H,W] or a list of those and returns new tensors
    of the same layout; ``from_logits`` takes the argmax first and returns class-id maps [B,1,D,H,W]."""

    def __init__(self, applied_labels: Union[Sequence[int], int], independent: bool = True, connectivity: Optional[int] = None):
        self.applied_labels = [applied_labels] if isinstance(applied_labels, int) else list(applied_labels)
        self.independent = independent
        self.connectivity = connectivity
        _connectivity(connectivity)

    def _batch(self, x, from_logits):
        return _ccl(x, self.connectivity, self.applied_labels, self.independent, from_logits, want_out=True)[0]

    def __call__(self, img, from_logits: bool = False):
        if isinstance(img, (list, tuple)):
            items = [t.unsqueeze(0) if t.dim() == 4 else t for t in img]
            if len({tuple(t.shape) for t in items}) == 1:                 # equal shapes: one call
                out = self._batch(torch.cat(items), from_logits)
                outs, i = [], 0
                for t in items:
                    outs.append(out[i:i + t.shape[0]])
                    i += t.shape[0]
            else:
                outs = [self._batch(t, from_logits) for t in items]
            return [o.squeeze(0) if t.dim() == 4 else o for o, t in zip(outs, img)]
        if img.dim() == 4:
            return self._batch(img.unsqueeze(0), from_logits).squeeze(0)
        return self._batch(img, from_logits)
