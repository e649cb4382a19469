"""GPU-resident training data: preprocessed volumes in HBM and the per-step random crops and augmentations of the reference's
training transforms (unetr_segmentation_3d.py:322-476; unetr_ranking_pretraining_3d.py:346-444), written straight into the
model's static input tensors with no host synchronisation, so one call can be replayed inside a captured graph:

    cache = VolumeCache(device)
    i = cache.add(image, label, scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True)   # CT: ScaleIntensityRanged + CropForegroundd
    aug = RandCropAugment(cache, spatial_size=96, num_samples=4, pos=1, neg=1)            # RandCropByPosNegLabeld + flips / rot90 / shift
    aug(x_static, y_static); step.run()

Kernels: csrc/augment.hip.  Semantics (MONAI 0.6.0) and the random-number assignment: DESIGN.md section 12 and
tests/augment_ref.py, which replays the params table of every call bit for bit on the CPU.  No CPU fallback.

``affine_prob > 0`` adds a random rotation and zoom per sample, taken at crop time from the whole cached volume in the same
single gather (trilinear image, nearest label, border padding); its semantics are this project's own (RandCropAugment's
docstring, DESIGN.md section 12, tests/augment_affine_ref.py).

``intensity=IntensityAugment(...)`` adds nnU-Net's intensity family on x after all of that: Gaussian blur, Gaussian noise,
brightness, contrast and gamma, flagged per sample, from the same Philox stream; again the project's own semantics
(IntensityAugment's and RandCropAugment's docstrings, DESIGN.md section 12, tests/augment_intensity_ref.py).

``sampling="label_classes"`` is MONAI's RandCropByLabelClassesd: the crop centre is a voxel of a class drawn by ratio, from
per-class voxel lists ``VolumeCache.build_class_indices`` builds on the GPU (map_classes_to_indices); the ratios live in device
memory (``aug.class_ratios``), so a captured call can be steered between replays (tests/augment_classes_ref.py).
"""
import ctypes
import dataclasses
import math
import struct
from typing import Optional, Sequence, Tuple, Union

import torch

from . import functional as Fn
from . import preprocess
from ._capi import AugAffineDesc, AugDesc, AugIntensityDesc, call, load

AFFINE_COLS = 16        # affine row (float32): flag, angle about spatial axis 0, 1, 2, zoom of axis 0, 1, 2, M [3][3] row-major
INTENSITY_COLS = 16     # intensity row (int32, floats as bits): flag bits, noise std, blur sigma of axis 0, 1, 2, brightness factor,
                        # contrast factor, gamma, low / high word of the call counter, six zeros
INTENSITY_NOISE, INTENSITY_BLUR, INTENSITY_BRIGHTNESS, INTENSITY_CONTRAST, INTENSITY_GAMMA = 1, 2, 4, 8, 16
MAX_BLUR_SIGMA = 2.0    # the blur's radius (int)(max(4 sigma, 0.5) + 0.5) stays within 8
_MAXDIM_AFFINE = 1 << 24  # volume extent up to which a float32 coordinate still names every voxel
PARAM_COLS = 8          # params row: volume, corner z, y, x, flip mask (bit a = spatial axis a), k, shift flag, offset (float bits)
_VCOLS = 12             # device volume table row: img ptr, lbl ptr, fg ptr, nfg, bg ptr, nbg, C, L, D, H, W, 0
_CCOLS = 2              # device class table row: concatenated class lists (int32) ptr, offsets (int64 [K + 1]) ptr
_MAXC = 8
_MAXS = 512
MAX_CLASSES = 32        # one bit per class in the list kernels
NORMALIZE_MODES = (None, "nonzero_channel_wise")
SAMPLING_MODES = ("pos_neg", "uniform", "label_classes")


class VolumeCache:
    """Preprocessed volumes resident on one device: images float32 [C, D, H, W], labels uint8 [L, D, H, W], each volume at its
    own shape, with its foreground / background voxel lists (monai map_binary_to_indices) and a device table of all of them."""

    def __init__(self, device, image_threshold: float = 0.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("3dmedicalimagesegmentation_amd: VolumeCache lives on a ROCm device; there is no CPU fallback.")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.image_threshold = float(image_threshold)
        self._vols = []          # (image, label, fg, bg)
        self.shapes = []         # (C, L, D, H, W) per volume
        self._affines = {}       # volume id -> 4x4 affine after add_raw's Spacing -> Orientation
        self._geometry = {}      # volume id -> preprocess.Geometry of add_raw (with the foreground crop): the way back
        self._origins = []       # per volume: (z0, y0, x0) of CropForegroundd's box on the grid add() was given
        self._table = None
        self._class_cfg = None   # (num_classes, image_mask) once build_class_indices was called
        self._classes = []       # per volume built so far: (lists int32, offsets int64 [K + 1] on the device, counts on the host)
        self._class_table = None

    def __len__(self):
        return len(self._vols)

    def add(self, image: torch.Tensor, label: torch.Tensor, scale_range: Optional[Sequence[float]] = None,
            crop_foreground: bool = False, scale_percentiles: Optional[Sequence[float]] = None) -> int:
        """ScaleIntensityRanged(a_min, a_max, b_min, b_max, clip=True) when scale_range is given, CropForegroundd(source_key=
        "image", margin=0) when crop_foreground, then the index lists; returns the volume's id.  May synchronise.
        scale_percentiles=(lower, upper, b_min, b_max): ScaleIntensityRangePercentilesd(lower, upper, b_min, b_max, clip=True,
        relative=False) as MONAI 0.6.0 is recalled to define it (parity-unpinned): a_min / a_max are the two percentiles of the
        whole image as given, before the foreground crop (topk_loss.percentile, rounded to float32), then the scale_range path."""
        if scale_percentiles is not None:
            if scale_range is not None:
                raise ValueError("scale_range and scale_percentiles exclude each other")
            lower, upper, pb_min, pb_max = (float(v) for v in scale_percentiles)
            if not (0.0 <= lower <= 100.0 and 0.0 <= upper <= 100.0):
                raise ValueError(f"scale_percentiles: percentages in [0, 100] expected, got {lower}, {upper}")
            if lower >= upper:
                raise ValueError(f"scale_percentiles: lower < upper expected, got {lower} >= {upper}")
        if image.dim() != 4 or label.dim() != 4 or image.shape[1:] != label.shape[1:]:
            raise ValueError(f"image [C,D,H,W] and label [L,D,H,W] with the same spatial shape expected, got "
                             f"{tuple(image.shape)} and {tuple(label.shape)}")
        C, L = image.shape[0], label.shape[0]
        D, H, W = image.shape[1:]
        if not (0 < C <= _MAXC and 0 < L <= _MAXC):
            raise ValueError(f"1..{_MAXC} image and label channels supported, got C={C}, L={L}")
        if D * H * W >= 2 ** 31:
            raise ValueError("volumes of at most 2**31 - 1 voxels are supported")
        dev = self.device
        with torch.cuda.device(dev):
            st = Fn._stream()
            img = image.detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()
            lbl = label.detach().to(device=dev, dtype=torch.float32).contiguous()
            mode, consts = 0, (0.0, 1.0, 1.0, 0.0, 0.0)
            if scale_percentiles is not None:
                from .topk_loss import percentile
                a_min, a_max = (struct.unpack("f", struct.pack("f", v))[0] for v in percentile(img, (lower, upper)).tolist())
                scale_range = (a_min, a_max, pb_min, pb_max)
            if scale_range is not None:
                a_min, a_max, b_min, b_max = (float(v) for v in scale_range)
                mode = 2 if a_max - a_min == 0.0 else 1
                consts = (a_min, a_max - a_min, b_max - b_min, b_min, b_max)   # float32 constants, as numpy casts them
            big = 0x7FFFFFFF
            box = torch.tensor([big, big, big, -1, -1, -1, 0], dtype=torch.int32, device=dev)
            call("unetr_aug_prep", img.data_ptr(), lbl.data_ptr(), C, L, D, H, W, mode, *consts, int(crop_foreground),
                 box.data_ptr(), box[6:].data_ptr(), st)
            b = box.tolist()
            if b[6]:
                raise ValueError("label values must be integers in 0..255")
            if crop_foreground:
                if b[3] < 0:
                    raise ValueError("CropForegroundd: the image has no voxel > 0, the foreground box is empty")
                z0, y0, x0 = b[0], b[1], b[2]
                d, h, w = b[3] - z0 + 1, b[4] - y0 + 1, b[5] - x0 + 1
            else:
                z0 = y0 = x0 = 0
                d, h, w = D, H, W
            oimg = torch.empty(C, d, h, w, dtype=torch.float32, device=dev)
            olbl = torch.empty(L, d, h, w, dtype=torch.uint8, device=dev)
            call("unetr_aug_crop", img.data_ptr(), lbl.data_ptr(), C, L, D, H, W, z0, y0, x0, d, h, w, oimg.data_ptr(),
                 olbl.data_ptr(), st)
            del img, lbl
            V = d * h * w
            nws = load().unetr_aug_index_ws_ints(V)
            ws = torch.empty(nws, dtype=torch.int32, device=dev)
            thr = self.image_threshold
            call("unetr_aug_index_count", oimg.data_ptr(), olbl.data_ptr(), C, L, V, thr, ws.data_ptr(), nws, st)
            nfg, nbg = ws[nws - 2:].tolist()
            if nfg == 0 and nbg == 0:
                raise ValueError("no sampling location available: the foreground and background index lists are both empty")
            fg = torch.empty(max(nfg, 1), dtype=torch.int32, device=dev)
            bg = torch.empty(max(nbg, 1), dtype=torch.int32, device=dev)
            call("unetr_aug_index_scatter", oimg.data_ptr(), olbl.data_ptr(), C, L, V, thr, ws.data_ptr(), nws, fg.data_ptr(),
                 bg.data_ptr(), st)
        self._vols.append((oimg, olbl, fg[:nfg], bg[:nbg]))
        self.shapes.append((C, L, d, h, w))
        self._origins.append((z0, y0, x0))
        self._table = None
        return len(self._vols) - 1

    def add_raw(self, image: torch.Tensor, label: torch.Tensor, affine, pixdim: Sequence[float] = (1.0, 1.0, 1.0),
                axcodes: str = "RAS", label_converter: Optional[str] = None, scale_range: Optional[Sequence[float]] = None,
                crop_foreground: bool = False) -> int:
        """A volume as LoadImaged leaves it (image [C, d0, d1, d2] float32 or int16, label [L, d0, d1, d2], both on the
        device, and the file's 4x4 affine): Spacingd(pixdim, mode=("bilinear", "nearest")) -> Orientationd(axcodes), with
        label_converter="brats" ConvertToMultiChannelBasedOnBratsClassesd on the label (preprocess.resample_orient), then add()."""
        img, lbl, new_affine = preprocess.resample_orient(image, label, affine, pixdim, axcodes, label_converter)
        i = self.add(img, lbl, scale_range=scale_range, crop_foreground=crop_foreground)
        self._affines[i] = new_affine
        geom = preprocess.geometry(image.shape[1:], affine, pixdim, axcodes)
        self._geometry[i] = geom.cropped(self._origins[i], self.shapes[i][2:])
        return i

    def affine(self, i: int):
        """4x4 float64 affine of a volume added with add_raw, as Orientationd leaves it: MONAI 0.6.0's CropForegroundd does
        not update the affine, so it describes the grid before the foreground crop."""
        if not 0 <= i < len(self._vols):
            raise IndexError(f"volume {i} out of range")
        if i not in self._affines:
            raise ValueError(f"volume {i} was added with add(): no affine is known")
        return self._affines[i].copy()

    def geometry(self, i: int) -> "preprocess.Geometry":
        """what add_raw's Spacing -> Orientation -> CropForeground did to volume i (preprocess.Geometry): the record
        ``restore`` needs to map a prediction back onto the scan's own voxel grid"""
        if not 0 <= i < len(self._vols):
            raise IndexError(f"volume {i} out of range")
        if i not in self._geometry:
            raise ValueError(f"volume {i} was added with add(): no affine is known")
        return self._geometry[i]

    def restore(self, i: int, pred: torch.Tensor, **kw) -> torch.Tensor:
        """preprocess.restore_native(pred, self.geometry(i), **kw): a prediction on volume i's grid -> the scan's native grid"""
        return preprocess.restore_native(pred, self.geometry(i), **kw)

    def image(self, i: int) -> torch.Tensor:
        return self._vols[i][0].unsqueeze(0)

    def label(self, i: int) -> torch.Tensor:
        return self._vols[i][1].unsqueeze(0)

    def fg_indices(self, i: int) -> torch.Tensor:
        return self._vols[i][2]

    def bg_indices(self, i: int) -> torch.Tensor:
        return self._vols[i][3]

    def table(self) -> torch.Tensor:
        """device int64 [n, 12] table of the volumes added so far (a fresh tensor after every add(), so an augment built
        earlier keeps its own table and its own set of volumes)"""
        if self._table is None:
            rows = []
            for (img, lbl, fg, bg), (C, L, D, H, W) in zip(self._vols, self.shapes):
                rows.append([img.data_ptr(), lbl.data_ptr(), fg.data_ptr(), fg.numel(), bg.data_ptr(), bg.numel(), C, L, D, H, W, 0])
            self._table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return self._table

    # ---------------------------------------------------------------- per-class voxel lists (RandCropByLabelClassesd)
    def build_class_indices(self, num_classes: Optional[int] = None, image_mask: bool = False) -> None:
        """monai map_classes_to_indices for every volume held, and lazily for volumes added later: one int32 list of voxel
        indices per class, ascending ravel order.  A single-channel label holds class ids: class c is ``label == c`` for c in
        0..num_classes-1 (required, 1..32), an id >= num_classes is in no list.  A label of L > 1 channels is one-hot or
        multi-label: class c is ``label[c] != 0``, num_classes must be None or L, lists may overlap.  ``image_mask`` keeps only
        voxels with any_c(image > image_threshold) (MONAI's image_key / image_threshold).  Costs 4 bytes per listed voxel:
        about one more image's worth per single-channel volume.  May synchronise; a second call with other arguments rebuilds."""
        if num_classes is not None and not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1..{MAX_CLASSES}, got {num_classes}")
        cfg = (None if num_classes is None else int(num_classes), bool(image_mask))
        for i, (_, L, *_dims) in enumerate(self.shapes):
            _class_count_of(L, cfg[0], f"volume {i}")
        if cfg != self._class_cfg:
            self._class_cfg, self._classes, self._class_table = cfg, [], None
        self._build_classes()

    def _build_classes(self) -> None:
        if self._class_cfg is None:
            raise ValueError("no class lists: call build_class_indices() first")
        num_classes, masked = self._class_cfg
        dev = self.device
        with torch.cuda.device(dev):
            st = Fn._stream()
            for i in range(len(self._classes), len(self._vols)):
                img, lbl = self._vols[i][:2]
                C, L, D, H, W = self.shapes[i]
                K, V = _class_count_of(L, num_classes, f"volume {i}"), D * H * W
                nws = load().unetr_aug_class_ws_ints(V, K)
                ws = torch.empty(nws, dtype=torch.int32, device=dev)
                offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
                args = (img.data_ptr(), lbl.data_ptr(), C, L, K, V, int(masked), self.image_threshold, ws.data_ptr(), nws,
                        offsets.data_ptr())
                call("unetr_aug_class_count", *args, st)
                off = offsets.tolist()
                lists = torch.empty(max(off[K], 1), dtype=torch.int32, device=dev)
                call("unetr_aug_class_scatter", *args, lists.data_ptr(), st)
                self._classes.append((lists, offsets, [off[c + 1] - off[c] for c in range(K)]))
                self._class_table = None

    def _class_record(self, i: int):
        if not 0 <= i < len(self._vols):
            raise IndexError(f"volume {i} out of range")
        self._build_classes()
        return self._classes[i]

    def class_indices(self, i: int, c: int) -> torch.Tensor:
        """device int32 list of the voxels of class c in volume i (a view of the volume's concatenated lists)"""
        lists, _, counts = self._class_record(i)
        if not 0 <= c < len(counts):
            raise IndexError(f"class {c} out of range")
        start = sum(counts[:c])
        return lists[start:start + counts[c]]

    def class_counts(self, i: int):
        """host list: the number of voxels of each class in volume i"""
        return list(self._class_record(i)[2])

    def class_offsets(self, i: int) -> torch.Tensor:
        """device int64 [K + 1]: where each class list starts in the concatenated array; the last entry is the total"""
        return self._class_record(i)[1]

    def class_table(self) -> torch.Tensor:
        """device int64 [n, 2] beside table(): pointer to the concatenated lists and to the offsets of every volume (a fresh
        tensor after every build)"""
        self._build_classes()
        if self._class_table is None:
            rows = [[lists.data_ptr(), offsets.data_ptr()] for lists, offsets, _ in self._classes]
            self._class_table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return self._class_table


def _class_count_of(L: int, num_classes: Optional[int], what: str) -> int:
    """K of a label with L channels under build_class_indices' rules"""
    if L == 1:
        if num_classes is None:
            raise ValueError(f"{what}: a single-channel label holds class ids, num_classes is required")
        return int(num_classes)
    if num_classes is not None and int(num_classes) != L:
        raise ValueError(f"{what}: a label of {L} channels has {L} classes, num_classes must be None or {L}, got {num_classes}")
    return L


def _triple(v, name):
    t = (v,) * 3 if isinstance(v, (int, float)) else tuple(v)
    if len(t) != 3:
        raise ValueError(f"{name}: one value or three (one per spatial axis) expected, got {v!r}")
    return t


def _bits_to_float(col: torch.Tensor) -> torch.Tensor:
    return col.to(torch.int32).contiguous().view(torch.float32)


@dataclasses.dataclass(frozen=True)
class IntensityAugment:
    """The intensity half of the augmentation, for ``RandCropAugment(..., intensity=...)``: per sample and with its own
    probability each, Gaussian blur (one sigma per spatial axis), Gaussian noise (std), brightness (x * f), contrast
    (clip((x - mean) * f + mean, min, max)) and gamma (((x - min) / (range + 1e-7)) ** gamma * range + min), applied in that
    order to x after everything else the augment does (normalize included); y is not touched.  Values are uniform in their
    ``(lo, hi)``; one set of draws serves all channels of a sample, statistics are per (sample, channel) over the crop.  These
    semantics are this project's own: nnU-Net's choice of operations, MONAI's formulas, no bit parity with either
    (tests/augment_intensity_ref.py).  Every probability defaults to 0: off."""
    noise_prob: float = 0.0
    noise_std: Tuple[float, float] = (0.0, 0.1)
    blur_prob: float = 0.0
    blur_sigma: Tuple[float, float] = (0.5, 1.0)
    brightness_prob: float = 0.0
    brightness_range: Tuple[float, float] = (0.75, 1.25)
    contrast_prob: float = 0.0
    contrast_range: Tuple[float, float] = (0.75, 1.25)
    gamma_prob: float = 0.0
    gamma_range: Tuple[float, float] = (0.7, 1.5)

    _OPS = (("noise_prob", "noise_std"), ("blur_prob", "blur_sigma"), ("brightness_prob", "brightness_range"),
            ("contrast_prob", "contrast_range"), ("gamma_prob", "gamma_range"))     # the order of the C descriptor

    def __post_init__(self):
        for pname, rname in self._OPS:
            p = float(getattr(self, pname))
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"{pname} must be in [0, 1], got {getattr(self, pname)}")
            try:
                lo, hi = (float(v) for v in getattr(self, rname))
            except (TypeError, ValueError):
                raise ValueError(f"{rname}: (low, high) expected, got {getattr(self, rname)!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"{rname}: finite bounds expected, got {getattr(self, rname)!r}")
            if lo > hi:
                raise ValueError(f"{rname}: low > high ({lo} > {hi})")
            if rname == "noise_std":
                if lo < 0:
                    raise ValueError(f"noise_std must be nonnegative, got {getattr(self, rname)!r}")
            elif lo <= 0:
                raise ValueError(f"{rname}: positive bounds expected, got {getattr(self, rname)!r}")
            if rname == "blur_sigma" and hi > MAX_BLUR_SIGMA:
                raise ValueError(f"blur_sigma must lie in (0, {MAX_BLUR_SIGMA}], got {getattr(self, rname)!r}")
            object.__setattr__(self, pname, p)
            object.__setattr__(self, rname, (lo, hi))

    @classmethod
    def nnunet(cls) -> "IntensityAugment":
        """nnU-Net's probabilities (noise 0.1, blur 0.2, brightness 0.15, contrast 0.15, gamma 0.3) with the default ranges"""
        return cls(noise_prob=0.1, blur_prob=0.2, brightness_prob=0.15, contrast_prob=0.15, gamma_prob=0.3)

    def _desc(self) -> AugIntensityDesc:
        d = AugIntensityDesc()
        for j, (pname, rname) in enumerate(self._OPS):
            d.prob[j] = getattr(self, pname)
            d.lo[j], d.hi[j] = getattr(self, rname)
        return d


class RandCropAugment:
    """One training batch per call: B // num_samples volumes from the schedule, num_samples crops of each (item-major, MONAI's
    list collate order), each followed by RandFlipd per axis, RandRotate90d, RandShiftIntensityd and optionally
    NormalizeIntensityd(nonzero=True, channel_wise=True).  ``aug(x, y)`` writes x [B, C, *S] and y [B, L, *S] (float32) and
    ``aug.params`` [B, 8] (int32) records what it drew.  Launches only, on the current stream; graph-capturable.

    ``affine_prob > 0`` takes each sample, with that probability, through a random rotation (``rotate_range``: one value or
    three, radians; the angle about spatial axis a is uniform in [-r_a, r_a]) and zoom (``zoom_range`` = (lo, hi), uniform; z > 1
    makes structures z times larger; ``zoom_per_axis`` draws one zoom per axis) and records it in ``aug.affine`` [B, 16]
    (float32: flag, 3 angles, 3 zooms, M row-major).  An output voxel goes back through rot90^k and the flips to crop position
    p as before; then, with c0 the crop corner and q = p - (S - 1) / 2, it reads the volume at
    ``c0 + (S - 1) / 2 + M q``,  ``M = R0(t0) R1(t1) R2(t2) diag(1 / z)``  (R2 turns (q0, q1); R0, R1 cyclically),
    trilinear for the image, nearest (floor(src + 0.5)) for the label.  The position is looked up in the whole cached volume, so
    real anatomy beside the crop comes into view; taps outside the volume take the nearest voxel (border padding).  Per sample:
    affine at crop time, flips, rot90, shift, normalize.  The crop corner is drawn as without the affine: the crop box lies in
    the volume, its warped footprint need not.  This is NOT bit parity with MONAI's RandAffined: that one warps the already
    cropped patch (so it pads where this reads the neighbouring anatomy), pads by reflection by default and orders and
    parametrises its matrix differently.  Unflagged samples are bit-identical to what ``affine_prob=0`` writes.

    ``intensity=IntensityAugment(...)`` adds, after all of the above and on x only, blur, noise, brightness, contrast and gamma
    in that order, each flagged per sample, and records the draws in ``aug.intensity`` [B, 16] (int32, float values as their
    bits: flag bits noise 1 / blur 2 / brightness 4 / contrast 8 / gamma 16, noise std, blur sigma of axis 0, 1, 2, brightness
    factor, contrast factor, gamma, low and high word of the call counter that keyed the draws, six zeros; an unflagged operation
    stores its neutral value).  The draws are Philox blocks 5..7 of the sample's stream, the noise of voxel group g of channel c
    is block (n, s, 16 + c, 1 + g); ``params`` and ``affine`` do not move.  These semantics are this project's own (nnU-Net's
    operations, MONAI's formulas, float32 in a fixed order: DESIGN.md section 12, tests/augment_intensity_ref.py), NOT bit
    parity with either.  With ``intensity=None`` the augment calls exactly the entry points it called before.

    ``sampling="label_classes"`` (RandCropByLabelClassesd) centres each crop on a voxel of a class drawn by ``class_ratios``
    (MONAI's ``ratios``; default all ones, nnU-Net's forced foreground over the classes present): ``num_classes`` is required
    (1..32) for a single-channel label of class ids and must be None or L for a label of L > 1 channels; ``class_image_mask``
    keeps only voxels with any_c(image > cache.image_threshold) (MONAI's image_key / image_threshold).  The lists come from
    ``cache.build_class_indices`` (4 bytes per listed voxel).  A class without voxels in the sample's volume has weight 0; the
    class is the first c with ``u * total < cum_c``.  Block 0 of the sample's Philox stream changes meaning in this mode only
    (word 0 the class, word 1 the voxel of that class), so with the same seed every column of ``params`` but the corner, and
    ``affine`` and ``intensity``, are what ``pos_neg`` writes.  ``aug.class_ratios`` [K] (float32, device) is read by the sampler
    on every call: ``set_class_ratios`` checks host values, or write it on the device between replays of a captured call.
    ``aug.classes`` [B] (int32) records the class drawn, -1 where no class was eligible and the corner was drawn uniformly.
    The other modes call exactly the entry points they called before."""

    def __init__(self, cache: VolumeCache, spatial_size: Union[int, Sequence[int]] = 96, num_samples: int = 4, pos: float = 1,
                 neg: float = 1, sampling: str = "pos_neg", flip_prob: Union[float, Sequence[float], None] = (0.1, 0.1, 0.1),
                 rot90_prob: float = 0.1, max_k: int = 3, spatial_axes: Tuple[int, int] = (0, 1),
                 shift_offsets: Union[float, Sequence[float]] = 0.1, shift_prob: float = 0.5, normalize: Optional[str] = None,
                 seed: int = 0, batch_size: Optional[int] = None, order_capacity: Optional[int] = None,
                 affine_prob: float = 0.0, rotate_range: Union[float, Sequence[float], None] = None,
                 zoom_range: Optional[Sequence[float]] = None, zoom_per_axis: bool = False,
                 intensity: Optional[IntensityAugment] = None, num_classes: Optional[int] = None, class_ratios=None,
                 class_image_mask: bool = False):
        if intensity is not None and not isinstance(intensity, IntensityAugment):
            raise ValueError(f"intensity must be an IntensityAugment or None, got {type(intensity).__name__}")
        S = tuple(int(s) for s in _triple(spatial_size, "spatial_size"))
        if any(not 0 < s <= _MAXS for s in S):
            raise ValueError(f"spatial_size must be in 1..{_MAXS} per axis, got {S}")
        if int(num_samples) < 1:
            raise ValueError(f"num_samples must be >= 1, got {num_samples}")
        B = int(num_samples if batch_size is None else batch_size)
        if B < 1 or B % int(num_samples):
            raise ValueError(f"batch_size ({B}) must be a positive multiple of num_samples ({num_samples})")
        if sampling not in SAMPLING_MODES:
            raise ValueError(f"sampling must be one of {SAMPLING_MODES}, got {sampling!r}")
        if sampling != "label_classes" and (num_classes is not None or class_ratios is not None or class_image_mask):
            raise ValueError('num_classes, class_ratios and class_image_mask belong to sampling="label_classes"')
        if pos < 0 or neg < 0:
            raise ValueError(f"pos and neg must be nonnegative, got pos={pos} neg={neg}")
        if pos + neg == 0:
            raise ValueError("Incompatible values: pos=0 and neg=0.")
        if normalize not in NORMALIZE_MODES:
            raise ValueError(f"normalize must be one of {NORMALIZE_MODES}, got {normalize!r}")
        ax = tuple(int(a) for a in spatial_axes)
        if len(ax) != 2 or ax[0] == ax[1] or any(not 0 <= a <= 2 for a in ax):
            raise ValueError(f"spatial_axes must be two different spatial axes in 0..2, got {spatial_axes!r}")
        if S[ax[0]] != S[ax[1]]:
            raise ValueError(f"RandRotate90d over axes {ax} needs equal crop sizes on them, got {S[ax[0]]} and {S[ax[1]]}")
        if int(max_k) < 1:
            raise ValueError(f"max_k must be >= 1, got {max_k}")
        fp = (0.0, 0.0, 0.0) if flip_prob is None else tuple(float(p) for p in _triple(flip_prob, "flip_prob"))
        if isinstance(shift_offsets, (int, float)):
            lo, hi = -abs(float(shift_offsets)), abs(float(shift_offsets))
        else:
            lo, hi = (float(v) for v in shift_offsets)
            if lo > hi:
                raise ValueError(f"shift_offsets: low > high ({lo} > {hi})")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must be in [0, 2**64)")
        if not 0.0 <= float(affine_prob) <= 1.0:
            raise ValueError(f"affine_prob must be in [0, 1], got {affine_prob}")
        if float(affine_prob) > 0 and rotate_range is None and zoom_range is None:
            raise ValueError("affine_prob > 0 needs rotate_range or zoom_range")
        rot = (0.0, 0.0, 0.0) if rotate_range is None else tuple(float(r) for r in _triple(rotate_range, "rotate_range"))
        if any(not (math.isfinite(r) and r >= 0) for r in rot):
            raise ValueError(f"rotate_range must be finite and nonnegative, got {rotate_range!r}")
        zlo, zhi = (1.0, 1.0) if zoom_range is None else (float(v) for v in zoom_range)
        if not (math.isfinite(zlo) and math.isfinite(zhi) and zlo > 0 and zhi > 0):
            raise ValueError(f"zoom_range: positive finite bounds expected, got {zoom_range!r}")
        if zlo > zhi:
            raise ValueError(f"zoom_range: low > high ({zlo} > {zhi})")
        shapes = list(cache.shapes)
        if not shapes:
            raise ValueError("the VolumeCache holds no volume")
        C, L = shapes[0][:2]
        for i, (c, l, *dims) in enumerate(shapes):
            if (c, l) != (C, L):
                raise ValueError(f"volume {i} has {c} image / {l} label channels, volume 0 has {C} / {L}")
            if any(d < s for d, s in zip(dims, S)):
                raise ValueError(f"volume {i} of spatial shape {tuple(dims)} is smaller than the crop {S}")
            if float(affine_prob) > 0 and any(d > _MAXDIM_AFFINE for d in dims):
                raise ValueError(f"volume {i} of spatial shape {tuple(dims)}: the affine gather supports extents up to 2**24")
        K = 0
        if sampling == "label_classes":
            if num_classes is not None and not 1 <= int(num_classes) <= MAX_CLASSES:
                raise ValueError(f"num_classes must be in 1..{MAX_CLASSES}, got {num_classes}")
            K = _class_count_of(L, num_classes, "sampling='label_classes'")
        n = len(shapes)
        cap = max(n, 4096) if order_capacity is None else int(order_capacity)
        if cap < n:
            raise ValueError(f"order_capacity ({cap}) must be at least the number of volumes ({n})")

        self.cache = cache
        self.spatial_size, self.num_samples, self.batch_size = S, int(num_samples), B
        self.sampling, self.pos_ratio = sampling, pos / (pos + neg)
        self.flip_prob, self.rot90_prob, self.max_k, self.spatial_axes = fp, float(rot90_prob), int(max_k), ax
        self.shift_range, self.shift_prob, self.normalize, self.seed = (lo, hi), float(shift_prob), normalize, int(seed)
        self.channels, self.label_channels, self.num_volumes = C, L, n
        self.affine_prob, self.rotate_range, self.zoom_range, self.zoom_per_axis = float(affine_prob), rot, (zlo, zhi), bool(zoom_per_axis)

        d = AugDesc()
        d.B, d.num_samples, d.C, d.L = B, self.num_samples, C, L
        d.S0, d.S1, d.S2 = S
        d.sampling = SAMPLING_MODES.index(sampling)
        d.ax0, d.ax1 = ax
        d.max_k, d.normalize = self.max_k, int(normalize is not None)
        d.pos_ratio = self.pos_ratio
        d.flip_prob[0], d.flip_prob[1], d.flip_prob[2] = fp
        d.rot90_prob, d.shift_prob, d.shift_lo, d.shift_hi = self.rot90_prob, self.shift_prob, lo, hi
        d.seed = self.seed
        self._desc = d

        dev = cache.device
        self.device = dev
        self._table = cache.table()            # this augment's volumes (kept alive by the cache)
        self._order = torch.zeros(cap, dtype=torch.int32, device=dev)
        self._order[:n] = torch.arange(n, dtype=torch.int32, device=dev)
        self._state = torch.tensor([0, 0, n, 0], dtype=torch.int64, device=dev)
        self.params = torch.zeros(B, PARAM_COLS, dtype=torch.int32, device=dev)
        self.affine = None                     # [B, 16] float32 once affine_prob > 0
        self._adesc = None
        ws = load().unetr_aug_gather_ws_bytes(ctypes.byref(d))
        if self.affine_prob > 0:
            a = AugAffineDesc()
            a.prob, a.zoom_lo, a.zoom_hi, a.zoom_per_axis = self.affine_prob, zlo, zhi, int(self.zoom_per_axis)
            a.rotate[0], a.rotate[1], a.rotate[2] = rot
            self._adesc = a
            self.affine = torch.zeros(B, AFFINE_COLS, dtype=torch.float32, device=dev)
            self.affine[:, [4, 5, 6, 7, 11, 15]] = 1.0
            ws = load().unetr_aug_gather_affine_ws_bytes(ctypes.byref(d))
        self._ws = torch.empty(max(ws, 8), dtype=torch.uint8, device=dev)
        self.intensity_config = intensity
        self.intensity = None                  # [B, 16] int32 once an IntensityAugment is given
        self._idesc = self._iws = None
        if intensity is not None:
            self._idesc = intensity._desc()
            self.intensity = torch.zeros(B, INTENSITY_COLS, dtype=torch.int32, device=dev)
            self.intensity[:, 5:8] = 0x3F800000                                     # 1.0f: the neutral factors and gamma
            self._iws = torch.empty(load().unetr_aug_intensity_ws_bytes(ctypes.byref(d)), dtype=torch.uint8, device=dev)
        self.num_classes = K
        self.class_ratios = self.classes = None    # [K] float32 (read by the sampler on every call) and [B] int32 in label_classes mode
        if K:
            cache.build_class_indices(num_classes=None if L > 1 else K, image_mask=class_image_mask)
            self._class_table = cache.class_table()
            self._class_records = [cache._class_record(i) for i in range(n)]       # keeps this augment's lists alive
            self.class_ratios = torch.ones(K, dtype=torch.float32, device=dev)
            self.classes = torch.full((B,), -1, dtype=torch.int32, device=dev)
            self.set_class_ratios(torch.ones(K) if class_ratios is None else class_ratios)

    # ---------------------------------------------------------------- schedule
    def set_order(self, ids) -> None:
        """volume schedule: item i of a call takes volume order[(cursor + i) % len(order)]; resets the cursor (device writes)"""
        ids = torch.as_tensor(ids).reshape(-1).to(torch.int64)
        h = ids.cpu()
        if h.numel() == 0 or h.numel() > self._order.numel():
            raise ValueError(f"order must hold 1..{self._order.numel()} volume ids (order_capacity), got {h.numel()}")
        if int(h.min()) < 0 or int(h.max()) >= self.num_volumes:
            raise ValueError(f"volume ids must be in 0..{self.num_volumes - 1}")
        self._order[:h.numel()].copy_(ids.to(device=self.device, dtype=torch.int32))
        self._state[1:3].copy_(torch.tensor([0, h.numel()], dtype=torch.int64))

    def set_class_ratios(self, ratios) -> None:
        """the class ratios of sampling="label_classes" (MONAI's ``ratios``): [K] nonnegative weights, copied into the device
        tensor ``class_ratios`` the sampler reads on every call, so a captured call follows them.  A host tensor or sequence is
        checked: length K, finite, nonnegative, and every volume must hold a class with a positive ratio.  A device tensor is
        copied without a synchronisation and unchecked: the sampler takes a negative or non-finite ratio as 0 and, for a
        volume left without an eligible class, draws the corner uniformly (``classes`` = -1)."""
        if self.class_ratios is None:
            raise ValueError('class ratios need an augment built with sampling="label_classes"')
        t = ratios if isinstance(ratios, torch.Tensor) else torch.as_tensor(ratios, dtype=torch.float32)
        if tuple(t.shape) != (self.num_classes,):
            raise ValueError(f"class_ratios: {self.num_classes} values (one per class) expected, got shape {tuple(t.shape)}")
        if not t.is_cuda:
            h = t.to(torch.float64)
            if not bool(torch.isfinite(h).all()) or bool((h < 0).any()):
                raise ValueError(f"class_ratios must be finite and nonnegative, got {h.tolist()}")
            for i, (_, _, counts) in enumerate(self._class_records):
                if not any(r > 0 and cnt > 0 for r, cnt in zip(h.tolist(), counts)):
                    raise ValueError(f"class_ratios {h.tolist()}: volume {i} holds no voxel of a class with a positive ratio "
                                     f"(class counts {counts})")
        self.class_ratios.copy_(t.to(device=self.device, dtype=torch.float32), non_blocking=True)

    def reset(self, call: int = 0) -> None:
        """set the device call counter (the Philox counter of the next call) and rewind the cursor"""
        self._state[0:2].copy_(torch.tensor([int(call), 0], dtype=torch.int64))

    @property
    def state(self) -> torch.Tensor:
        """device int64 [4]: call counter, cursor, len(order), 0"""
        return self._state

    @property
    def order(self) -> torch.Tensor:
        return self._order

    # ---------------------------------------------------------------- per step
    def _check_out(self, x, y):
        Fn._require_gpu(x)
        Fn._require_gpu(y)
        S, B = self.spatial_size, self.batch_size
        if tuple(x.shape) != (B, self.channels, *S) or tuple(y.shape) != (B, self.label_channels, *S):
            raise ValueError(f"x [{B},{self.channels},{S[0]},{S[1]},{S[2]}] and y [{B},{self.label_channels},{S[0]},{S[1]},{S[2]}] "
                             f"expected, got {tuple(x.shape)} and {tuple(y.shape)}")
        if not (x.is_contiguous() and y.is_contiguous()):
            raise ValueError("x and y must be contiguous")
        if x.device != self.device or y.device != self.device:
            raise ValueError(f"x and y must live on {self.device}")

    def __call__(self, x: torch.Tensor, y: torch.Tensor) -> None:
        self._check_out(x, y)
        st = Fn._stream()
        d = ctypes.byref(self._desc)
        if self.intensity is not None:         # before the sampler: it reads the call counter the sampler then advances
            call("unetr_aug_intensity_sample", d, ctypes.byref(self._idesc), self._state.data_ptr(), self.intensity.data_ptr(), st)
        if self.classes is not None:
            a = None if self.affine is None else ctypes.byref(self._adesc)
            call("unetr_aug_sample_classes", d, a, self._table.data_ptr(), self.num_volumes, self._class_table.data_ptr(),
                 self.num_classes, self.class_ratios.data_ptr(), self._order.data_ptr(), self._state.data_ptr(),
                 self.params.data_ptr(), None if self.affine is None else self.affine.data_ptr(), self.classes.data_ptr(), st)
        if self.affine is None:
            if self.classes is None:
                call("unetr_aug_sample", d, self._table.data_ptr(), self.num_volumes, self._order.data_ptr(), self._state.data_ptr(),
                     self.params.data_ptr(), st)
            call("unetr_aug_gather", d, self._table.data_ptr(), self.num_volumes, self.params.data_ptr(), x.data_ptr(),
                 y.data_ptr(), self._ws.data_ptr(), self._ws.numel(), st)
        else:
            if self.classes is None:
                call("unetr_aug_sample_affine", d, ctypes.byref(self._adesc), self._table.data_ptr(), self.num_volumes,
                     self._order.data_ptr(), self._state.data_ptr(), self.params.data_ptr(), self.affine.data_ptr(), st)
            call("unetr_aug_gather_affine", d, self._table.data_ptr(), self.num_volumes, self.params.data_ptr(),
                 self.affine.data_ptr(), x.data_ptr(), y.data_ptr(), self._ws.data_ptr(), self._ws.numel(), st)
        if self.intensity is not None:
            call("unetr_aug_intensity_apply", d, self.intensity.data_ptr(), x.data_ptr(), self._iws.data_ptr(), self._iws.numel(), st)

    def _check_intensity(self, table: torch.Tensor) -> None:
        if self.intensity is None:
            raise ValueError("an intensity table needs an augment built with intensity=IntensityAugment(...)")
        if tuple(table.shape) != (self.batch_size, INTENSITY_COLS):
            raise ValueError(f"intensity [{self.batch_size}, {INTENSITY_COLS}] expected, got {tuple(table.shape)}")
        if table.is_cuda:
            return
        h = table.to(torch.int32)
        flags = h[:, 0]
        if not bool(((flags >= 0) & (flags <= 31)).all()):
            raise ValueError("intensity: the flag bits (column 0) must be in 0..31")
        v = _bits_to_float(h[:, 1:8])
        if not bool(torch.isfinite(v).all()):
            raise ValueError("intensity: every value must be finite")
        if bool((v[:, 0] < 0).any()):
            raise ValueError("intensity: the noise std (column 1) must be nonnegative")
        blur = (flags & INTENSITY_BLUR) != 0
        if bool((v[:, 1:4] > MAX_BLUR_SIGMA).any()) or bool((v[:, 1:4] < 0).any()) or bool((v[blur, 1:4] <= 0).any()):
            raise ValueError(f"intensity: a blur sigma (columns 2..4) must lie in (0, {MAX_BLUR_SIGMA}] (0 on a row without blur)")
        if bool((v[:, 4:7] <= 0).any()):
            raise ValueError("intensity: brightness factor, contrast factor and gamma (columns 5..7) must be positive")

    def apply(self, params: torch.Tensor, x: torch.Tensor, y: torch.Tensor, affine: Optional[torch.Tensor] = None,
              intensity: Optional[torch.Tensor] = None) -> None:
        """the gather alone with an explicit [B, 8] table (int32) and, on an augment built with affine_prob > 0, an explicit
        [B, 16] affine table (float32; None: no sample is flagged); host tables are checked (crop inside the volume, affine
        values finite, flag 0 or 1).  On an augment built with an IntensityAugment, an explicit [B, 16] intensity table (int32,
        the layout of ``aug.intensity``; None: no operation is flagged) is followed by the intensity passes; a host table is
        checked (flag bits 0..31, values finite, std >= 0, sigma <= 2 and > 0 where blur is flagged, factors and gamma > 0)."""
        self._check_out(x, y)
        if intensity is not None:
            self._check_intensity(intensity)
        if affine is not None:
            if self.affine is None:
                raise ValueError("an affine table needs an augment built with affine_prob > 0")
            if tuple(affine.shape) != (self.batch_size, AFFINE_COLS):
                raise ValueError(f"affine [{self.batch_size}, {AFFINE_COLS}] expected, got {tuple(affine.shape)}")
            if not affine.is_cuda:
                h = affine.to(torch.float32)
                if not bool(torch.isfinite(h).all()):
                    raise ValueError("affine: every value must be finite")
                if not bool(((h[:, 0] == 0) | (h[:, 0] == 1)).all()):
                    raise ValueError("affine: the flag (column 0) must be 0 or 1")
        if tuple(params.shape) != (self.batch_size, PARAM_COLS):
            raise ValueError(f"params [{self.batch_size}, {PARAM_COLS}] expected, got {tuple(params.shape)}")
        if not params.is_cuda:
            for r in params.to(torch.int64).tolist():
                if not 0 <= r[0] < self.num_volumes:
                    raise ValueError(f"params row {r}: volume out of range")
                dims = self.cache.shapes[r[0]][2:]
                if any(c < 0 or c + s > dm for c, s, dm in zip(r[1:4], self.spatial_size, dims)):
                    raise ValueError(f"params row {r}: the crop leaves the volume {tuple(dims)}")
        p = params.to(device=self.device, dtype=torch.int32).contiguous()
        if affine is None:
            call("unetr_aug_gather", ctypes.byref(self._desc), self._table.data_ptr(), self.num_volumes, p.data_ptr(),
                 x.data_ptr(), y.data_ptr(), self._ws.data_ptr(), self._ws.numel(), Fn._stream())
        else:
            a = affine.to(device=self.device, dtype=torch.float32).contiguous()
            call("unetr_aug_gather_affine", ctypes.byref(self._desc), self._table.data_ptr(), self.num_volumes, p.data_ptr(),
                 a.data_ptr(), x.data_ptr(), y.data_ptr(), self._ws.data_ptr(), self._ws.numel(), Fn._stream())
        if intensity is not None:
            t = intensity.to(device=self.device, dtype=torch.int32).contiguous()
            call("unetr_aug_intensity_apply", ctypes.byref(self._desc), t.data_ptr(), x.data_ptr(), self._iws.data_ptr(),
                 self._iws.numel(), Fn._stream())
