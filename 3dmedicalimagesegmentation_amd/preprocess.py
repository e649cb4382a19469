"""Per-volume front of the reference's transform chain on the GPU (unetr_segmentation_3d.py:326-331, 383-388, 413-419, 465-471):

    Spacingd(pixdim, mode=("bilinear", "nearest")) -> Orientationd(axcodes)      [BraTS: ConvertToMultiChannelBasedOnBratsClassesd first]

Both transforms are affine maps on voxel indices, so ``plan`` folds them on the host (float64, numpy only) into one 3x4 matrix
and ``resample_orient`` runs one HIP gather (csrc/preprocess.hip): trilinear for the image, round-half-even nearest for the label,
border clamping, MONAI 0.6.0 semantics (align_corners=False, diagonal=False) as restated in tests/preprocess_ref.py and
DESIGN.md section 13.  ``VolumeCache.add_raw`` puts it in front of ``VolumeCache.add``.  No CPU fallback.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as Fn
from ._capi import call

LABEL_CONVERTERS = (None, "brats")
_MAXC = 8
_AXCODE_LABELS = (("L", "R"), ("P", "A"), ("I", "S"))


def _io_orientation(affine: np.ndarray) -> np.ndarray:
    """nibabel.io_orientation: row i = (output axis closest to input axis i, +1 / -1), input axes served in order"""
    rzs = affine[:3, :3]
    zooms = np.sqrt((rzs * rzs).sum(0))
    zooms[zooms == 0] = 1.0
    P, S, Qs = np.linalg.svd(rzs / zooms, full_matrices=False)
    keep = S > S.max() * 3 * np.finfo(S.dtype).eps
    R = P[:, keep] @ Qs[keep]
    ornt = np.full((3, 2), np.nan)
    for i in range(3):
        col = R[:, i]
        if not np.allclose(col, 0):
            a = int(np.argmax(np.abs(col)))
            ornt[i] = (a, -1.0 if col[a] < 0 else 1.0)
            R[a, :] = 0
    return ornt


def _axcodes_ornt(axcodes) -> np.ndarray:
    codes = tuple(axcodes)
    if len(codes) != 3:
        raise ValueError(f"axcodes must name three axes, got {axcodes!r}")
    ornt = np.zeros((3, 2))
    for i, code in enumerate(codes):
        hit = [(a, -1.0 if code == lo else 1.0) for a, (lo, hi) in enumerate(_AXCODE_LABELS) if code in (lo, hi)]
        if not hit:
            raise ValueError(f"axcodes: {code!r} is not one of L, R, P, A, I, S")
        ornt[i] = hit[0]
    if sorted(ornt[:, 0]) != [0, 1, 2]:
        raise ValueError(f"axcodes must name every axis once, got {axcodes!r}")
    return ornt


def plan(shape: Sequence[int], affine, pixdim: Sequence[float] = (1.0, 1.0, 1.0), axcodes: str = "RAS"
         ) -> Tuple[Tuple[int, int, int], np.ndarray, np.ndarray]:
    """The host half of Spacing -> Orientation for a volume of spatial ``shape`` with the 4x4 ``affine``: returns the output
    shape, the 3x4 float64 matrix that maps an output voxel index (j, 1) to its source index (before clamping), and the affine
    of the output.  Where MONAI's Spacing finds its transform within 1e-3 of the identity it copies the data; the matrix is
    then the exact flip / transpose of the Orientation step alone."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or any(s < 1 for s in shape):
        raise ValueError(f"three positive spatial extents expected, got {shape}")
    A = np.array(affine.detach().cpu().numpy() if isinstance(affine, torch.Tensor) else affine, dtype=np.float64)
    if A.shape != (4, 4):
        raise ValueError(f"affine must be 4x4, got {A.shape}")
    pix = np.array(pixdim, dtype=np.float64).reshape(-1)
    if pix.shape != (3,) or not np.all(np.isfinite(pix)) or np.any(pix <= 0):
        raise ValueError(f"pixdim must be three positive numbers, got {pixdim!r}")
    if not np.all(np.isfinite(A)) or np.linalg.matrix_rank(A) < 4:
        raise ValueError("affine is singular or not finite")
    dst = _axcodes_ornt(axcodes)

    # Spacing: zoom_affine(diagonal=False) rescales the columns to pixdim; compute_shape_offset (same-orientation branch)
    norm = np.sqrt(np.sum(np.square(A), 0))[:3]
    A_new = A @ np.diag(np.append(pix / norm, 1.0))
    corners = np.array(np.meshgrid(*[(0.0, s - 1.0) for s in shape], indexing="ij")).reshape(3, -1)
    corners = A @ np.concatenate((corners, np.ones_like(corners[:1])))
    corners = np.linalg.inv(A_new) @ corners
    corners = corners[:3] / corners[3]
    sp_shape = np.round(np.ptp(corners, axis=1) + 1.0).astype(int)
    A_new[:3, 3] = (A[:, 3] / A[3, 3])[:3]
    T = np.linalg.inv(A) @ A_new
    if np.allclose(T, np.eye(4), atol=1e-3):
        T, sp_shape = np.eye(4), np.array(shape)

    # Orientation: flips and a transpose as the index map in = M @ out on the resampled grid
    src = _io_orientation(A_new)
    if np.isnan(src).any():
        raise ValueError("affine is singular: an axis has no direction")
    M = np.zeros((4, 4))
    M[3, 3] = 1.0
    out_shape = [0, 0, 0]
    for i in range(3):
        j = int(np.nonzero(dst[:, 0] == src[i, 0])[0][0])      # output axis that shows input axis i
        flip = src[i, 1] * dst[j, 1]
        M[i, j] = flip
        if flip < 0:
            M[i, 3] = sp_shape[i] - 1
        out_shape[j] = int(sp_shape[i])
    return tuple(out_shape), np.ascontiguousarray((T @ M)[:3]), A_new @ M


def resample_orient(image: torch.Tensor, label: Optional[torch.Tensor], affine, pixdim: Sequence[float] = (1.0, 1.0, 1.0),
                    axcodes: str = "RAS", label_converter: Optional[str] = None):
    """image [C, d0, d1, d2] (float32 or int16; other types are cast to float32) and label [L, d0, d1, d2] or None (integer
    values 0..255) on a ROCm device -> (image' float32 [C, D, H, W], label' uint8 [L, D, H, W] or None, new affine 4x4 float64
    numpy).  label_converter="brats" takes a one-channel label and writes the four channels ==0, 2|3, 1|2|3, ==3."""
    if label_converter not in LABEL_CONVERTERS:
        raise ValueError(f"label_converter must be one of {LABEL_CONVERTERS}, got {label_converter!r}")
    for t in (image, label):
        if t is not None and not t.is_cuda:
            raise RuntimeError("3dmedicalimagesegmentation_amd: the HIP backend needs tensors on a ROCm device "
                               "(got a CPU tensor); there is no CPU fallback.")
    if image.dim() != 4 or not 0 < image.shape[0] <= _MAXC:
        raise ValueError(f"image [C, d0, d1, d2] with 1..{_MAXC} channels expected, got {tuple(image.shape)}")
    if label is not None:
        if label.dim() != 4 or label.shape[1:] != image.shape[1:] or label.device != image.device:
            raise ValueError(f"label [L, d0, d1, d2] on the image's device and grid expected, got {tuple(label.shape)} on "
                             f"{label.device} for an image {tuple(image.shape)} on {image.device}")
        if label_converter == "brats" and label.shape[0] != 1:
            raise ValueError(f"label_converter='brats' takes a one-channel label, got {label.shape[0]} channels")
        if not 0 < label.shape[0] <= _MAXC:
            raise ValueError(f"1..{_MAXC} label channels supported, got {label.shape[0]}")
    n = tuple(image.shape[1:])
    out_shape, mat, new_affine = plan(n, affine, pixdim, axcodes)
    if n[0] * n[1] * n[2] >= 2 ** 31 or out_shape[0] * out_shape[1] * out_shape[2] >= 2 ** 31:
        raise ValueError("volumes of at most 2**31 - 1 voxels (source and resampled) are supported")
    dev = image.device
    with torch.cuda.device(dev):
        img = image.detach()
        if img.dtype not in (torch.float32, torch.int16):
            img = img.to(torch.float32)
        img = img.contiguous()
        C, L, lbl, olbl = img.shape[0], 0, None, None
        if label is not None:
            lbl = label.detach()
            if lbl.dtype != torch.uint8:
                ok = (lbl >= 0) & (lbl <= 255)
                if lbl.is_floating_point():
                    ok &= lbl == lbl.round()
                if not bool(ok.all()):
                    raise ValueError("label values must be integers in 0..255")
                lbl = lbl.to(torch.uint8)
            lbl = lbl.contiguous()
            L = 4 if label_converter == "brats" else lbl.shape[0]
            olbl = torch.empty(L, *out_shape, dtype=torch.uint8, device=dev)
        oimg = torch.empty(C, *out_shape, dtype=torch.float32, device=dev)
        m = (ctypes.c_double * 12)(*mat.reshape(-1).tolist())
        call("unetr_resample_orient", img.data_ptr(), int(img.dtype == torch.int16), lbl.data_ptr() if lbl is not None else None,
             C, L, int(label_converter == "brats"), n[0], n[1], n[2], m, out_shape[0], out_shape[1], out_shape[2], oimg.data_ptr(),
             olbl.data_ptr() if olbl is not None else None, Fn._stream())
    return oimg, olbl, new_affine
