"""The segmentation loss family behind MONAI's names: ``loss = lambda_region * R + lambda_voxel * X`` with R one of Dice, Jaccard,
Tversky and generalized Dice and X one of cross entropy and sigmoid focal loss, computed by the HIP kernels in csrc/seg_loss.hip (one
streaming pass forward, one backward, whatever the variant).  ``SegLoss`` is the general form; ``DiceLoss``, ``TverskyLoss``,
``GeneralizedDiceLoss``, ``FocalLoss`` and ``DiceFocalLoss`` are presets with MONAI's argument names.  DiceCELoss with the options
losses.DiceCELoss refuses is ``SegLoss(region="dice", voxel="ce", ...)``.  Mean reduction only.  No CPU fallback."""
import torch
import torch.nn as nn

from . import functional as Fn
from . import loss_common as lc

_REGION = {"none": 0, "dice": 1, "jaccard": 2, "tversky": 3, "generalized_dice": 4}
_VOXEL = {"none": 0, "ce": 1, "focal": 2}
_W_TYPE = {"square": 0, "simple": 1, "uniform": 2}


class SegLoss(nn.Module):
    """Two input forms, as DiceCELoss has them:
      * ``to_onehot_y=True, softmax=True``: target [B,1,*spatial] class ids, probabilities = channel softmax;
      * ``to_onehot_y=False, sigmoid=True``: target [B,C,*spatial] float mask, probabilities = sigmoid.
    A loss without region term and with ``voxel="focal"`` reads the raw logits only and takes either target form without an
    activation.  ``ignore_index`` (class-id targets only): voxels with that label count nowhere; every call needs at least one
    other voxel.  ``class_weight`` has one entry per channel (the background included) and weighs the voxel term."""

    def __init__(self, region: str = "dice", voxel: str = "ce", include_background: bool = True, to_onehot_y: bool = False,
                 softmax: bool = False, sigmoid: bool = False, squared_pred: bool = False, batch: bool = False,
                 smooth_nr: float = 1e-5, smooth_dr: float = 1e-5, alpha: float = 0.5, beta: float = 0.5, w_type: str = "square",
                 gamma: float = 2.0, class_weight=None, ignore_index=None, lambda_region: float = 1.0, lambda_voxel: float = 1.0,
                 reduction: str = "mean") -> None:
        super().__init__()
        if region not in _REGION:
            raise ValueError(f"region={region!r}: expected one of {sorted(_REGION)}")
        if voxel not in _VOXEL:
            raise ValueError(f"voxel={voxel!r}: expected one of {sorted(_VOXEL)}")
        if w_type not in _W_TYPE:
            raise ValueError(f"w_type={w_type!r}: expected one of {sorted(_W_TYPE)}")
        if region == "none" and voxel == "none":
            raise ValueError("region='none' and voxel='none': the loss has no term")
        lc.require_mean(reduction)
        multilabel = lc.activation_form(to_onehot_y, softmax, sigmoid, required=region != "none" or voxel == "ce")
        if squared_pred and region in ("tversky", "generalized_dice"):
            raise NotImplementedError(f"squared_pred=True is not defined for region={region!r}")
        if ignore_index is not None and multilabel:
            raise NotImplementedError("ignore_index needs class-id targets (to_onehot_y=True)")
        if class_weight is not None:
            if voxel == "none":
                raise ValueError("class_weight weighs the voxel term, and voxel='none'")
            if voxel == "ce" and multilabel:
                raise NotImplementedError("class_weight with voxel='ce' needs class-id targets (to_onehot_y=True)")
            class_weight = lc.class_weight_list(class_weight)
        self.region, self.voxel = region, voxel
        self.class_weight = class_weight
        self.cfg = dict(multilabel=int(multilabel), region=_REGION[region], voxel=_VOXEL[voxel],
                        include_background=int(bool(include_background)), squared_pred=int(bool(squared_pred)), batch=int(bool(batch)),
                        w_type=_W_TYPE[w_type], has_ignore=int(ignore_index is not None),
                        ignore_index=int(ignore_index) if ignore_index is not None else 0,
                        smooth_nr=float(smooth_nr), smooth_dr=float(smooth_dr), alpha=float(alpha), beta=float(beta), gamma=float(gamma),
                        lambda_region=float(lambda_region) if region != "none" else 0.0,
                        lambda_voxel=float(lambda_voxel) if voxel != "none" else 0.0)
        self._cw = {}      # device -> class_weight as a device buffer, created at first use

    def _check(self, input, target):
        lc.check_call(input, target, self.cfg, self.class_weight)

    def _weights(self, device):
        return lc.weights_on(self._cw, self.class_weight, device)

    def terms(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """3-vector (loss, region term, voxel term), the terms before their lambdas; only element 0 carries gradient."""
        self._check(input, target)
        return Fn.SegLossFn.apply(input, target, self.cfg, self._weights(input.device))

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self._check(input, target)
        return Fn.SegLossFn.apply(input, target, self.cfg, self._weights(input.device), True)


def _activation(name, to_onehot_y, softmax, sigmoid, other_act):
    if other_act is not None:
        raise NotImplementedError(f"{name}: other_act is not implemented")
    return dict(to_onehot_y=to_onehot_y, softmax=softmax, sigmoid=sigmoid)


class DiceLoss(SegLoss):
    def __init__(self, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False, softmax: bool = False,
                 other_act=None, squared_pred: bool = False, jaccard: bool = False, reduction: str = "mean", smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, batch: bool = False) -> None:
        super().__init__(region="jaccard" if jaccard else "dice", voxel="none", include_background=include_background,
                         squared_pred=squared_pred, batch=batch, smooth_nr=smooth_nr, smooth_dr=smooth_dr, reduction=reduction,
                         **_activation("DiceLoss", to_onehot_y, softmax, sigmoid, other_act))


class TverskyLoss(SegLoss):
    def __init__(self, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False, softmax: bool = False,
                 other_act=None, alpha: float = 0.5, beta: float = 0.5, reduction: str = "mean", smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, batch: bool = False) -> None:
        super().__init__(region="tversky", voxel="none", include_background=include_background, alpha=alpha, beta=beta, batch=batch,
                         smooth_nr=smooth_nr, smooth_dr=smooth_dr, reduction=reduction,
                         **_activation("TverskyLoss", to_onehot_y, softmax, sigmoid, other_act))


class GeneralizedDiceLoss(SegLoss):
    def __init__(self, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False, softmax: bool = False,
                 other_act=None, w_type: str = "square", reduction: str = "mean", smooth_nr: float = 1e-5, smooth_dr: float = 1e-5,
                 batch: bool = False) -> None:
        super().__init__(region="generalized_dice", voxel="none", include_background=include_background, w_type=w_type, batch=batch,
                         smooth_nr=smooth_nr, smooth_dr=smooth_dr, reduction=reduction,
                         **_activation("GeneralizedDiceLoss", to_onehot_y, softmax, sigmoid, other_act))


class FocalLoss(SegLoss):
    """sigmoid focal loss of the raw logits; ``weight`` has one entry per channel"""

    def __init__(self, include_background: bool = True, to_onehot_y: bool = False, gamma: float = 2.0, weight=None,
                 reduction: str = "mean", ignore_index=None) -> None:
        super().__init__(region="none", voxel="focal", include_background=include_background, to_onehot_y=to_onehot_y, gamma=gamma,
                         class_weight=weight, ignore_index=ignore_index, reduction=reduction)


class DiceFocalLoss(SegLoss):
    def __init__(self, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False, softmax: bool = False,
                 other_act=None, squared_pred: bool = False, jaccard: bool = False, reduction: str = "mean", smooth_nr: float = 1e-5,
                 smooth_dr: float = 1e-5, batch: bool = False, gamma: float = 2.0, focal_weight=None, lambda_dice: float = 1.0,
                 lambda_focal: float = 1.0, ignore_index=None) -> None:
        super().__init__(region="jaccard" if jaccard else "dice", voxel="focal", include_background=include_background,
                         squared_pred=squared_pred, batch=batch, smooth_nr=smooth_nr, smooth_dr=smooth_dr, gamma=gamma,
                         class_weight=focal_weight, ignore_index=ignore_index, lambda_region=lambda_dice, lambda_voxel=lambda_focal,
                         reduction=reduction, **_activation("DiceFocalLoss", to_onehot_y, softmax, sigmoid, other_act))
