"""Binary morphology and hole filling of a discrete prediction, on the device:

    mask = binary_closing(klcc(inferer(x, net, post="argmax")), iterations=2)
    mask = binary_fill_holes(mask)
    ids = FillHoles(applied_labels=[1, 2])(class_id_map)

``binary_dilation`` / ``binary_erosion`` / ``binary_opening`` / ``binary_closing`` follow the functions of the same names in
scipy.ndimage with ``structure=generate_binary_structure(3, connectivity)``, ``binary_contour`` is ``m & ~binary_erosion(m)``,
``binary_fill_holes`` is scipy's per (item, channel), ``FillHoles`` is the fill_holes rule of MONAI on a class-id map.  Every
channel of ``x`` ([B,C,D,H,W] or a decollated [C,D,H,W]; float32, uint8 or bool) is its own mask, set where the value is != 0;
the result is a new tensor of the same shape and dtype that holds 0 or 1.  The masks are packed to one bit per voxel and stepped
in that form by the kernels of csrc/morphology.hip (unetr_morph, unetr_fill_holes); the hole filling labels the background with
``connected_components``.  Stream-ordered launches, no host synchronisation: the calls can sit inside a captured graph.  Not
offered: arbitrary structuring elements, ``mask=``, ``origin=``, ``iterations < 1`` (repeat until nothing changes) and
grey-scale morphology.  Semantics are restated in DESIGN.md section 22.  No CPU fallback.
"""
from typing import Optional, Sequence, Union

import torch

from . import functional as Fn
from ._capi import call, load
from .postprocess import _applied_mask, _connectivity, connected_components

MORPH_TILE = 8        # = MORPH_T of csrc/morphology.hip: rows along z and along y a workgroup owns
MORPH_FUSED = 4       # = MORPH_K: iterations one launch runs in LDS; n iterations take ceil(n / MORPH_FUSED) launches
_MAX_EXTENT = 1024
_MAX_CHANNELS = 16
_MAX_PLANES = 65535
_INT_MAX = 2 ** 31 - 1
_DILATE, _ERODE, _OPEN, _CLOSE, _CONTOUR = range(5)


def _check_connectivity(connectivity):
    if connectivity is None:
        raise ValueError("connectivity should be 1, 2 or 3, got None")
    return _connectivity(connectivity)


def _check_iterations(iterations):
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise ValueError(f"iterations should be an integer >= 1, got {iterations!r}")
    if iterations < 1:
        raise ValueError(f"iterations should be >= 1, got {iterations}: scipy's iterations < 1 (repeat until nothing changes) "
                         "needs a decision on the host and is not offered")
    return iterations


def _check_border(border_value):
    if isinstance(border_value, bool) or border_value not in (0, 1):
        raise ValueError(f"border_value should be 0 or 1, got {border_value!r}")
    return int(border_value)


def _masks(x, what):
    """(x as a contiguous [B,C,D,H,W] float32 / uint8 tensor on the device, whether the caller's was 4-D)"""
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise ValueError("3-D volumes [B,C,D,H,W] or [C,D,H,W] expected")
    if x.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise ValueError(f"{what}: float32, uint8 or bool expected, got {x.dtype}")
    if x.numel() == 0:
        raise ValueError("empty input")
    squeeze = x.dim() == 4
    if squeeze:
        x = x.unsqueeze(0)
    B, C, D, H, W = x.shape
    if C > _MAX_CHANNELS or max(D, H, W) > _MAX_EXTENT or D * H * W >= _INT_MAX or B * C > _MAX_PLANES:
        raise NotImplementedError(f"{what}: at most {_MAX_CHANNELS} channels, {_MAX_EXTENT} voxels along each axis, 2^31 - 2 "
                                  f"voxels per volume and {_MAX_PLANES} masks (got B={B}, C={C}, {D}x{H}x{W})")
    bits = x.view(torch.uint8) if x.dtype == torch.bool else x
    Fn._require_gpu(bits, ids=True)
    return bits.contiguous(), squeeze


def _result(out, x, squeeze):
    if x.dtype == torch.bool:
        out = out.view(torch.bool)
    return out.squeeze(0) if squeeze else out


def _morph(x, op, iterations, connectivity, border_value, what, class_id=-1):
    """one unetr_morph call; class_id >= 0 takes the mask ``x == class_id`` of a class-id map instead of ``x != 0``"""
    conn = _check_connectivity(connectivity)
    bits, squeeze = _masks(x, what)
    B, C, D, H, W = bits.shape
    out = torch.empty_like(bits)
    ws = torch.empty(load().unetr_morph_workspace_bytes(D, H, W, B * C), dtype=torch.uint8, device=bits.device)
    call("unetr_morph", bits.data_ptr(), out.data_ptr(), int(bits.dtype == torch.uint8), B, C, D, H, W, class_id, op, iterations,
         conn, border_value, ws.data_ptr(), ws.numel(), Fn._stream())
    return _result(out, x, squeeze)


def binary_dilation(x: torch.Tensor, iterations: int = 1, connectivity: int = 1, border_value: int = 0) -> torch.Tensor:
    """scipy.ndimage.binary_dilation(m, generate_binary_structure(3, connectivity), iterations, border_value=border_value) of
    every mask of x; ``border_value`` is what the voxels outside the volume read as"""
    return _morph(x, _DILATE, _check_iterations(iterations), connectivity, _check_border(border_value), "binary_dilation")


def binary_erosion(x: torch.Tensor, iterations: int = 1, connectivity: int = 1, border_value: int = 0) -> torch.Tensor:
    """scipy.ndimage.binary_erosion, as ``binary_dilation``; with the default ``border_value=0`` the volume's faces erode"""
    return _morph(x, _ERODE, _check_iterations(iterations), connectivity, _check_border(border_value), "binary_erosion")


def binary_opening(x: torch.Tensor, iterations: int = 1, connectivity: int = 1) -> torch.Tensor:
    """scipy.ndimage.binary_opening: ``iterations`` erosions, then as many dilations, both with border_value 0"""
    return _morph(x, _OPEN, _check_iterations(iterations), connectivity, 0, "binary_opening")


def binary_closing(x: torch.Tensor, iterations: int = 1, connectivity: int = 1) -> torch.Tensor:
    """scipy.ndimage.binary_closing: ``iterations`` dilations, then as many erosions, both with border_value 0 -- so a mask
    that reaches a face of the volume is eroded there, exactly as scipy's result is"""
    return _morph(x, _CLOSE, _check_iterations(iterations), connectivity, 0, "binary_closing")


def binary_contour(x: torch.Tensor, connectivity: int = 1) -> torch.Tensor:
    """the voxels of every mask that one erosion (border_value 0) removes: ``m & ~binary_erosion(m, connectivity=...)``"""
    return _morph(x, _CONTOUR, 1, connectivity, 0, "binary_contour")


def _fill(x, connectivity, class_map, applied, what):
    bits, squeeze = _masks(x, what)
    B, C, D, H, W = bits.shape
    # the background's components; a hole is one that touches none of the six faces
    labels = connected_components((bits == 0).to(torch.float32), connectivity)
    out = torch.empty_like(bits)
    ws = torch.empty(load().unetr_fill_holes_workspace_bytes(D, H, W, B * C, class_map), dtype=torch.uint8, device=bits.device)
    call("unetr_fill_holes", bits.data_ptr(), out.data_ptr(), int(bits.dtype == torch.uint8), labels.data_ptr(), B, C, D, H, W,
         class_map, applied, connectivity, ws.data_ptr(), ws.numel(), Fn._stream())
    return _result(out, x, squeeze)


def binary_fill_holes(x: torch.Tensor, connectivity: int = 1) -> torch.Tensor:
    """scipy.ndimage.binary_fill_holes(m, generate_binary_structure(3, connectivity)) of every mask of x: the mask plus every
    component of its complement (components taken under ``connectivity``) that touches none of the volume's six faces"""
    return _fill(x, _check_connectivity(connectivity), 0, 0, "binary_fill_holes")


class FillHoles:
    """The fill_holes rule of MONAI on a class-id map [B,1,D,H,W] (or a decollated [1,D,H,W]; float32 or uint8, integral ids
    0..31): a component of the background ``x == 0``, labelled under ``connectivity`` (None = 3), that touches no face of the
    volume and whose voxels' neighbours under the same connectivity carry exactly one non-zero id l is set to l, when l is in
    ``applied_labels`` (None = every id).  Everything else keeps its value; the result is a new tensor."""

    def __init__(self, applied_labels: Optional[Union[Sequence[int], int]] = None, connectivity: Optional[int] = None):
        self.applied_labels = applied_labels
        self.connectivity = connectivity
        self._conn = _connectivity(connectivity)
        self._applied = _applied_mask(applied_labels, 0, 1)

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        if not isinstance(img, torch.Tensor) or img.dim() not in (4, 5) or img.shape[-4] != 1:
            raise ValueError("FillHoles: a class-id map [B,1,D,H,W] or [1,D,H,W] expected")
        if img.dtype == torch.bool:
            raise ValueError("FillHoles: a class-id map is float32 or uint8, got torch.bool")
        return _fill(img, self._conn, 1, self._applied, "FillHoles")
