"""Per-volume front of the reference's transform chain on the GPU (unetr_segmentation_3d.py:326-331, 383-388, 413-419, 465-471):

    Spacingd(pixdim, mode=("bilinear", "nearest")) -> Orientationd(axcodes)      [BraTS: ConvertToMultiChannelBasedOnBratsClassesd first]

Both transforms are affine maps on voxel indices, so ``plan`` folds them on the host (float64, numpy only) into one 3x4 matrix
and ``resample_orient`` runs one HIP gather (csrc/preprocess.hip): trilinear for the image, round-half-even nearest for the label,
border clamping, MONAI 0.6.0 semantics (align_corners=False, diagonal=False) as restated in tests/preprocess_ref.py and
DESIGN.md section 13.  ``VolumeCache.add_raw`` puts it in front of ``VolumeCache.add``.  No CPU fallback.

The way back: ``geometry`` records what ``plan`` decided (and ``VolumeCache.add_raw`` the foreground crop), and ``restore_native``
maps a prediction on the cropped 1 mm grid onto the scan's own voxel grid with one HIP gather (csrc/restore.hip): the inverse of
Spacingd -> Orientationd -> CropForegroundd, with argmax / sigmoid threshold / the BraTS label rule fused in (DESIGN.md section 17,
restated in tests/restore_ref.py).
"""
import ctypes
import dataclasses
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as Fn
from ._capi import RestoreGeom, call

LABEL_CONVERTERS = (None, "brats")
RESTORE_MODES = ("nearest", "linear")
RESTORE_POST = {None: 0, "argmax": 1, "sigmoid": 2}
_MAXC = 8
_RESTORE_MAXC = 16
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


# ---------------------------------------------------------------- the way back: native grid <- cropped 1 mm grid
def _frozen(a, shape):
    a = np.array(a, dtype=np.float64).reshape(shape)
    a.setflags(write=False)
    return a


@dataclasses.dataclass(frozen=True, eq=False)
class Geometry:
    """What Spacing -> Orientation -> CropForeground did to one scan, as far as the way back needs it (host, float64):

    native_shape      (n0, n1, n2) of the file
    affine            the file's 4x4 affine (what a NIfTI of the restored mask is written with)
    pixdim, axcodes   as given to ``plan``
    full_shape        the resampled and oriented grid before any crop
    forward           4x4 ``T @ M`` exactly as ``plan`` decided it (``T = I`` under the copy rule): native index = forward @ [j, 1]
    oriented_affine   the affine after Orientation (``VolumeCache.affine``)
    crop_origin, crop_shape   the foreground box on the full grid; origin 0 and the full shape when there was no crop
    """
    native_shape: Tuple[int, int, int]
    affine: np.ndarray
    pixdim: Tuple[float, float, float]
    axcodes: str
    full_shape: Tuple[int, int, int]
    forward: np.ndarray
    oriented_affine: np.ndarray
    crop_origin: Tuple[int, int, int]
    crop_shape: Tuple[int, int, int]

    def cropped(self, origin: Sequence[int], shape: Sequence[int]) -> "Geometry":
        """a copy whose box is ``origin`` .. ``origin + shape - 1`` of the full grid; nothing else changes"""
        o, s = tuple(int(v) for v in origin), tuple(int(v) for v in shape)
        if len(o) != 3 or len(s) != 3 or any(a < 0 or b < 1 or a + b > f for a, b, f in zip(o, s, self.full_shape)):
            raise ValueError(f"crop box origin {o} shape {s} does not lie inside the grid {self.full_shape}")
        return dataclasses.replace(self, crop_origin=o, crop_shape=s)

    def native_spacing(self) -> Tuple[float, float, float]:
        """voxel sizes of the file's own grid (the column norms of ``affine[:3, :3]``) in the file's axis order: the ``spacing``
        that goes with a ``restore_native`` mask.  ``pixdim`` is the spacing of the resampled grid."""
        return tuple(float(v) for v in np.sqrt((self.affine[:3, :3] ** 2).sum(axis=0)))

    def inverse_matrix(self) -> np.ndarray:
        """3x4 float64: native index (i, 1) -> coordinate on the full resampled grid, the exact inverse of ``forward`` (MONAI
        0.6.0's Spacingd.inverse resamples with inv(new_affine) @ old_affine).  A scan that was copied forward (an all-integer
        ``forward``: a signed permutation with integer offsets) has an all-integer inverse and is copied back."""
        inv = np.linalg.inv(self.forward)
        if np.array_equal(self.forward, np.rint(self.forward)) and np.abs(inv - np.rint(inv)).max() < 1e-9:
            inv = np.rint(inv) + 0.0                    # + 0.0: no negative zeros
        return np.ascontiguousarray(inv[:3])


def geometry(shape: Sequence[int], affine, pixdim: Sequence[float] = (1.0, 1.0, 1.0), axcodes: str = "RAS") -> Geometry:
    """the Geometry of a volume of spatial ``shape`` with the 4x4 ``affine`` under ``plan(shape, affine, pixdim, axcodes)``, uncropped"""
    out_shape, mat, new_affine = plan(shape, affine, pixdim, axcodes)
    A = np.array(affine.detach().cpu().numpy() if isinstance(affine, torch.Tensor) else affine, dtype=np.float64)
    return Geometry(native_shape=tuple(int(s) for s in shape), affine=_frozen(A, (4, 4)),
                    pixdim=tuple(float(p) for p in np.array(pixdim, dtype=np.float64).reshape(-1)), axcodes="".join(axcodes),
                    full_shape=tuple(out_shape), forward=_frozen(np.vstack([mat, [0.0, 0.0, 0.0, 1.0]]), (4, 4)),
                    oriented_affine=_frozen(new_affine, (4, 4)), crop_origin=(0, 0, 0), crop_shape=tuple(out_shape))


def restore_native(pred: torch.Tensor, geometry: Geometry, mode: str = "nearest", post: Optional[str] = None,
                   label_converter: Optional[str] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A prediction on the (cropped) resampled grid -> the scan's own voxel grid: the inverse of CropForegroundd, Orientationd
    and Spacingd in one gather.  pred [C, d, h, w] or [1, C, d, h, w] with (d, h, w) = geometry.crop_shape, float32 (what
    SlidingWindowInferer returns for every ``post``) or, for mode="nearest", uint8 (cache labels); C <= 16.

        mode="nearest"                    [C, n0, n1, n2] of pred's dtype: the picked voxel (class ids, one-hot, multi-label)
        mode="linear"                     float32 [C, ...]: trilinear scores
        mode="linear", post="argmax"      uint8 [1, ...] class ids, first maximal channel; the C-channel volume is never stored
        mode="linear", post="sigmoid"     uint8 [C, ...]: interpolated logit >= 0
        ... + label_converter="brats"     (any discrete result of the 4 channels BG / TC / WT / ET) uint8 [1, ...] label map:
                                          1 where WT, then 2 where TC, then 3 where ET, else 0

    Native voxels whose nearest grid point lies outside the crop box are background: 0 in every output.  ``out`` receives the
    result when given (contiguous, on pred's device).  Launches one kernel on the current stream; no host synchronisation."""
    if not isinstance(geometry, Geometry):
        raise ValueError(f"geometry must be a preprocess.Geometry, got {type(geometry).__name__}")
    if mode not in RESTORE_MODES:
        raise ValueError(f"mode must be one of {RESTORE_MODES}, got {mode!r}")
    if post not in RESTORE_POST:
        raise ValueError(f"post must be one of {list(RESTORE_POST)}, got {post!r}")
    if label_converter not in LABEL_CONVERTERS:
        raise ValueError(f"label_converter must be one of {LABEL_CONVERTERS}, got {label_converter!r}")
    if post is not None and mode == "nearest":
        raise ValueError(f"post={post!r} reduces interpolated scores: it needs mode='linear'")
    if pred.dim() == 5:
        if pred.shape[0] != 1:
            raise ValueError(f"one scan per call (each has its own geometry), got a batch of {pred.shape[0]}")
        pred = pred[0]
    if pred.dim() != 4:
        raise ValueError(f"pred [C, d, h, w] or [1, C, d, h, w] expected, got {tuple(pred.shape)}")
    C = pred.shape[0]
    if tuple(pred.shape[1:]) != tuple(geometry.crop_shape):
        raise ValueError(f"pred's spatial shape {tuple(pred.shape[1:])} is not the geometry's crop shape {tuple(geometry.crop_shape)}")
    if not 0 < C <= _RESTORE_MAXC:
        raise ValueError(f"1..{_RESTORE_MAXC} channels supported, got {C}")
    linear, brats = mode == "linear", label_converter == "brats"
    if pred.dtype != torch.float32 and not (pred.dtype == torch.uint8 and not linear):
        raise ValueError(f"pred must be float32 (or uint8 with mode='nearest'), got {pred.dtype} with mode={mode!r}")
    if brats and C != 4:
        raise ValueError(f"label_converter='brats' takes the 4 channels background / TC / WT / ET, got {C}")
    if brats and linear and post is None:
        raise ValueError("label_converter='brats' needs a discrete result: mode='nearest', or post='argmax' / 'sigmoid'")
    n = tuple(geometry.native_shape)
    if n[0] * n[1] * n[2] >= 2 ** 31 or int(np.prod(geometry.full_shape, dtype=np.int64)) >= 2 ** 31:
        raise ValueError("volumes of at most 2**31 - 1 voxels (native and resampled) are supported")
    out_dtype = torch.uint8 if (post is not None or brats) else pred.dtype
    out_shape = (1 if (brats or post == "argmax") else C, *n)
    if out is not None:
        if tuple(out.shape) != out_shape or out.dtype != out_dtype:
            raise ValueError(f"out {list(out_shape)} of {out_dtype} expected, got {list(out.shape)} of {out.dtype}")
        if not out.is_contiguous() or out.device != pred.device:
            raise ValueError("out must be contiguous and on pred's device")
    if not pred.is_cuda:
        raise RuntimeError("3dmedicalimagesegmentation_amd: the HIP backend needs tensors on a ROCm device "
                           "(got a CPU tensor); there is no CPU fallback.")
    g = RestoreGeom()
    g.m[:] = geometry.inverse_matrix().reshape(-1).tolist()
    g.full[:], g.origin[:], g.crop[:] = geometry.full_shape, geometry.crop_origin, geometry.crop_shape
    with torch.cuda.device(pred.device):
        src = pred.detach().contiguous()
        if out is None:
            out = torch.empty(out_shape, dtype=out_dtype, device=pred.device)
        call("unetr_restore_native", src.data_ptr(), int(src.dtype == torch.uint8), C, g, n[0], n[1], n[2], int(linear),
             RESTORE_POST[post], int(brats), out.data_ptr(), Fn._stream())
    return out
