"""MI355X-native UNETR training hot path (gfx950 HIP kernels behind the reference's nn.Module interface).

The directory name starts with a digit, so import it with
``importlib.import_module("3dmedicalimagesegmentation_amd")`` -- or put this directory itself on
``sys.path`` and keep the reference scripts' own ``from unetr import UNETR`` line unchanged.
"""
from .unetr import UNETR, UNETRLogits, default_precision  # noqa: F401
from .losses import DiceCELoss, ranking_loss  # noqa: F401
from .seg_losses import DiceFocalLoss, DiceLoss, FocalLoss, GeneralizedDiceLoss, SegLoss, TverskyLoss  # noqa: F401
from .distance import BoundaryLoss, HausdorffDTLoss, distance_transform_edt, signed_distance_map  # noqa: F401
from .topk_loss import DiceTopKLoss, TopKLoss, kth_value, percentile  # noqa: F401
from .optim import AdamW  # noqa: F401
from .grad_clip import clip_grad_norm_  # noqa: F401
from .inference import DiceMetric, SlidingWindowInferer, sliding_window_inference  # noqa: F401
from .metrics import (ConfusionMatrixMetric, HausdorffDistanceMetric, SurfaceDiceMetric, SurfaceDistanceMetric,  # noqa: F401
                      surface_metrics)
from .postprocess import KeepLargestConnectedComponent, connected_components, remove_small_components  # noqa: F401
from .morphology import (FillHoles, binary_closing, binary_contour, binary_dilation, binary_erosion, binary_fill_holes,  # noqa: F401
                         binary_opening)
from .lesion_metrics import LesionWiseMetric, lesion_wise_metrics, panoptic_quality  # noqa: F401
from .train_step import TrainStep  # noqa: F401
from .augment import IntensityAugment, RandCropAugment, VolumeCache  # noqa: F401
from .preprocess import Geometry, resample_orient, restore_native  # noqa: F401
from .functional import invalidate_weight_shadows, refresh_derived_weights  # noqa: F401
from . import _capi, augment, ddp, distance, functional, grad_clip, inference, lesion_metrics, metrics, morphology, postprocess, preprocess, seg_losses, topk_loss, train_step  # noqa: F401

__all__ = ["UNETR", "UNETRLogits", "DiceCELoss", "ranking_loss", "AdamW", "default_precision", "sliding_window_inference",
           "SlidingWindowInferer", "DiceMetric", "ConfusionMatrixMetric", "HausdorffDistanceMetric", "TrainStep", "invalidate_weight_shadows",
           "refresh_derived_weights",
           "VolumeCache", "RandCropAugment", "IntensityAugment", "resample_orient", "restore_native", "Geometry", "KeepLargestConnectedComponent", "connected_components",
           "remove_small_components", "surface_metrics", "SurfaceDistanceMetric", "SurfaceDiceMetric",
           "SegLoss", "DiceLoss", "TverskyLoss", "GeneralizedDiceLoss", "FocalLoss", "DiceFocalLoss",
           "distance_transform_edt", "signed_distance_map", "BoundaryLoss", "HausdorffDTLoss",
           "TopKLoss", "DiceTopKLoss", "kth_value", "percentile",
           "binary_dilation", "binary_erosion", "binary_opening", "binary_closing", "binary_contour", "binary_fill_holes", "FillHoles",
           "clip_grad_norm_", "lesion_wise_metrics", "LesionWiseMetric", "panoptic_quality"]
