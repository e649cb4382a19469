"""Euclidean distance transforms on the device and the two losses that train on them: ``BoundaryLoss`` (Kervadec et al. 2019) and
``HausdorffDTLoss`` (Karimi & Salcudean 2019, MONAI's name), computed by the HIP kernels in csrc/edt.hip and csrc/dist_loss.hip.
Every call is a fixed sequence of launches on the current stream -- no host synchronisation, scratch from ``functional.workspace`` --
so the losses sit inside a captured training step.  ``distance_transform_edt`` is scipy.ndimage's function of that name for volumes
that already live on the GPU.  Extents up to 512 per axis, up to 16 channels.  No CPU fallback."""
import ctypes

import torch
import torch.nn as nn

from . import functional as Fn
from . import loss_common as lc
from ._capi import DistLossDesc, EdtDesc, call, call_rc

_FORM = {"mask": 0, "mask_u8": 1, "class_ids": 2, "softmax": 3, "sigmoid": 4}
_FIELD = {"distance": 0, "signed": 1, "unsigned": 2}
_KIND = {"boundary": 0, "hausdorff": 1}


def _spacing(spacing):
    if spacing is None:
        return None
    s = tuple(float(v) for v in (spacing.tolist() if isinstance(spacing, torch.Tensor) else spacing))
    if len(s) != 3 or not all(0.0 < v < float("inf") for v in s):
        raise ValueError(f"spacing={spacing!r}: expected three positive voxel sizes (z, y, x)")
    return s


def _edt(src, form, B, C, S, field, spacing=None, squared=False, alpha=1.0, out=None, accumulate=False):
    """one unetr_edt call: `src` (contiguous, on the device) read in `form`, the field written to (or added into) `out` [B,C,*S]"""
    if len(S) != 3:
        raise ValueError(f"three spatial dimensions expected, got {tuple(S)}")
    d = EdtDesc(B=B, C=C, D=S[0], H=S[1], W=S[2], form=_FORM[form], field=_FIELD[field], squared=int(bool(squared)),
                accumulate=int(bool(accumulate)), has_spacing=int(spacing is not None), alpha=float(alpha))
    if spacing is not None:
        d.spacing = (ctypes.c_float * 3)(*spacing)
    if out is None:
        out = torch.empty((B, C) + tuple(S), dtype=torch.float32, device=src.device)
    ws = Fn.workspace(src.device)
    rc = call_rc("unetr_edt", ctypes.byref(d), src.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 4, Fn._stream())
    if rc != 0:
        raise NotImplementedError(f"the HIP distance transform takes up to 16 channels and extents up to 512; got C={C}, spatial {tuple(S)}")
    return out


def distance_transform_edt(mask: torch.Tensor, spacing=None, squared: bool = False) -> torch.Tensor:
    """scipy.ndimage.distance_transform_edt(mask, sampling=spacing) on the device: for every voxel the Euclidean distance to the
    nearest voxel where ``mask`` is 0, float32, shaped like ``mask`` ([*S], [N,*S] or [B,C,*S] with three spatial dimensions; each
    volume on its own).  ``squared=True`` returns the squared distance -- without a spacing an exact integer value.  A volume
    without a zero is +inf everywhere (scipy leaves arbitrary values there)."""
    if mask.dim() not in (3, 4, 5):
        raise ValueError(f"mask must be [*S], [N,*S] or [B,C,*S] with three spatial dimensions, got {tuple(mask.shape)}")
    if mask.numel() == 0:
        raise ValueError("mask is empty")
    S = tuple(mask.shape[-3:])
    B, C = (1, 1) if mask.dim() == 3 else (mask.shape[0], 1) if mask.dim() == 4 else tuple(mask.shape[:2])
    if mask.dtype == torch.float32:
        src, form = mask, "mask"
    else:
        src = mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0
        src, form = src.contiguous().view(torch.uint8), "mask_u8"
    Fn._require_gpu(src, ids=True)
    return _edt(src.contiguous(), form, B, C, S, "distance", _spacing(spacing), squared).view(mask.shape)


def signed_distance_map(target: torch.Tensor, num_classes=None, spacing=None, unsigned: bool = False) -> torch.Tensor:
    """The distance field of every channel's object, [B,C,*S] float32.  ``num_classes=C``: ``target`` holds class ids [B,1,*S] and
    channel c is the object ``target == c``; ``num_classes=None``: ``target`` is a multilabel mask [B,C,*S] (object = non-zero).
    With d_fg / d_bg the distance to the nearest voxel of / outside the object:
      signed (the boundary loss's):    d_fg outside the object, -(d_bg - u) inside it, u = 1 voxel or the smallest spacing;
      unsigned (the Hausdorff-DT's):   d_fg + d_bg.
    An object that is empty or fills the volume has no boundary in view: its field is 0 everywhere."""
    if target.dim() != 5:
        raise ValueError(f"target must be [B,1,*S] class ids or a [B,C,*S] mask with three spatial dimensions, got {tuple(target.shape)}")
    Fn._require_gpu(target)
    target = target.contiguous()
    if num_classes is not None:
        if target.shape[1] != 1:
            raise ValueError("target must be [B,1,*spatial] class indices when num_classes is given")
        form, C = "class_ids", int(num_classes)
    else:
        form, C = "mask", target.shape[1]
    return _edt(target, form, target.shape[0], C, tuple(target.shape[2:]), "unsigned" if unsigned else "signed", _spacing(spacing))


def prediction_distance_map(logits: torch.Tensor, sigmoid: bool = False, spacing=None) -> torch.Tensor:
    """the unsigned field of the thresholded prediction, as HausdorffDTLoss sees it: channel softmax (or sigmoid) of ``logits``
    [B,C,*S] > 0.5, derived inside the kernel"""
    if logits.dim() != 5:
        raise ValueError(f"logits must be [B,C,*S] with three spatial dimensions, got {tuple(logits.shape)}")
    Fn._require_gpu(logits)
    logits = logits.contiguous()
    return _edt(logits, "sigmoid" if sigmoid else "softmax", logits.shape[0], logits.shape[1], tuple(logits.shape[2:]), "unsigned",
                _spacing(spacing))


class DistLossFn(torch.autograd.Function):
    """forward: the field of the target (and, for the Hausdorff-DT loss, of the thresholded prediction, accumulated into the same
    tensor) by unetr_edt, then unetr_distloss_fwd; backward: one unetr_distloss_bwd launch.  The field is an ordinary torch
    allocation, saved for backward; `weight` is the one-element device tensor both kernels read."""

    @staticmethod
    def forward(ctx, logits, target, weight, cfg, spacing, alpha):
        Fn._require_gpu(logits)
        if logits.dim() != 5:
            raise ValueError(f"logits must be [B,C,*S] with three spatial dimensions, got {tuple(logits.shape)}")
        ml = cfg["multilabel"]
        logits, target, B, C, V = Fn._loss_inputs(logits, target, ml)
        S = tuple(logits.shape[2:])
        tform = "mask" if ml else "class_ids"
        if cfg["kind"] == _KIND["boundary"]:
            field = _edt(target, tform, B, C, S, "signed", spacing)
        else:
            field = _edt(target, tform, B, C, S, "unsigned", spacing, alpha=alpha)
            _edt(logits, "sigmoid" if ml else "softmax", B, C, S, "unsigned", spacing, alpha=alpha, out=field, accumulate=True)
        d = DistLossDesc(B=B, C=C, V=V, **cfg)
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        ws = Fn.workspace(logits.device)
        call("unetr_distloss_fwd", ctypes.byref(d), logits.data_ptr(), target.data_ptr(), field.data_ptr(), weight.data_ptr(),
             out.data_ptr(), ws.data_ptr(), ws.numel() * 4, Fn._stream())
        ctx.save_for_backward(logits, target, field, weight)
        ctx.desc = d
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        logits, target, field, weight = ctx.saved_tensors
        dloss = dout.reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        call("unetr_distloss_bwd", ctypes.byref(ctx.desc), logits.data_ptr(), target.data_ptr(), field.data_ptr(), weight.data_ptr(),
             dloss.data_ptr(), dlogits.data_ptr(), Fn._stream())
        return dlogits, None, None, None, None, None


class _DistanceLoss(nn.Module):
    """Two input forms, as SegLoss has them:
      * ``to_onehot_y=True, softmax=True``: target [B,1,*spatial] class ids, probabilities = channel softmax;
      * ``to_onehot_y=False, sigmoid=True``: target [B,C,*spatial] float mask, probabilities = sigmoid.
    ``weight`` multiplies the loss and lives in device memory (``.weight``, one float32): ``set_weight`` changes it without a
    synchronisation, also between the replays of a captured step.  ``spacing`` = voxel size (z, y, x) of the distance fields."""
    _kind = None

    def __init__(self, alpha, include_background, to_onehot_y, softmax, sigmoid, spacing, weight, reduction):
        super().__init__()
        lc.require_mean(reduction)
        multilabel = lc.activation_form(to_onehot_y, softmax, sigmoid)
        if not float(alpha) > 0.0:
            raise ValueError(f"alpha={alpha!r}: expected a positive exponent")
        self.alpha = float(alpha)
        self.spacing = _spacing(spacing)
        self.cfg = dict(multilabel=int(multilabel), kind=_KIND[self._kind], include_background=int(bool(include_background)))
        self.register_buffer("weight", lc.device_scalar(weight), persistent=False)

    def set_weight(self, w: float) -> None:
        """write the device scalar (a fill launch on the current stream, no synchronisation)"""
        self.weight.fill_(float(w))

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        lc.check_call(input, target, self.cfg)
        weight = lc.scalar_on(self, "weight", input, "the loss weight")
        return DistLossFn.apply(input, target, weight, self.cfg, self.spacing, self.alpha)


class BoundaryLoss(_DistanceLoss):
    """``weight * mean(p * phi_G)`` over (batch, included channels, voxels): phi_G is the signed distance field of the target
    (``signed_distance_map``), negative inside the object, so probability mass is pulled inside the boundary."""
    _kind = "boundary"

    def __init__(self, include_background: bool = False, to_onehot_y: bool = False, softmax: bool = False, sigmoid: bool = False,
                 spacing=None, weight: float = 1.0, reduction: str = "mean") -> None:
        super().__init__(1.0, include_background, to_onehot_y, softmax, sigmoid, spacing, weight, reduction)


class HausdorffDTLoss(_DistanceLoss):
    """``weight * mean((p - g)^2 * (F_P^alpha + F_G^alpha))`` over (batch, included channels, voxels): F_G and F_P are the unsigned
    distance fields of the target and of the prediction thresholded at 0.5; F_P is a constant of the gradient."""
    _kind = "hausdorff"

    def __init__(self, alpha: float = 2.0, include_background: bool = False, to_onehot_y: bool = False, softmax: bool = False,
                 sigmoid: bool = False, spacing=None, weight: float = 1.0, reduction: str = "mean") -> None:
        super().__init__(alpha, include_background, to_onehot_y, softmax, sigmoid, spacing, weight, reduction)
