"""CPU restatement (float64) of the way back from the cropped 1 mm grid to a scan's own voxel grid: MONAI 0.6.0's
CropForegroundd.inverse (zero padding back to the full grid), Orientationd.inverse and Spacingd.inverse (a resampling with
inv(new_affine) @ old_affine, border padding) as remembered from their sources (not pinned against their output), folded into
the one formula csrc/restore.hip implements.  For every native voxel i:

    s = clamp(Minv @ [i, 1], 0, full - 1)           Minv = inverse of the forward T @ M of tests/preprocess_ref.py
    r = rint(s), half to even; r outside the crop box on any axis -> background, every output 0
    nearest  x[r - origin]
    linear   the eight taps floor(s), floor(s) + 1 clamped INTO the box, weights from s

It builds on preprocess_ref's source_coords / tie_mask; with no crop it is preprocess_ref.fused_gather with the inverse matrix.
"""
import numpy as np

import preprocess_ref as R


def as4x4(m):
    m = np.asarray(m, dtype=np.float64)
    return m if m.shape == (4, 4) else np.vstack([m.reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def coords(minv, native_shape, full_shape):
    """float64 [n0*n1*n2, 3]: where every native voxel lies on the full resampled grid, clamped to it (border padding)"""
    return R.source_coords(as4x4(minv), native_shape, full_shape)


def inside_mask(minv, native_shape, full_shape, origin, crop):
    """[n0*n1*n2] bool: rint(s) lies inside the crop box on every axis"""
    r = np.rint(coords(minv, native_shape, full_shape)).astype(int)
    o, c = np.asarray(origin), np.asarray(crop)
    return ((r >= o) & (r < o + c)).all(1)


def ties(minv, native_shape, full_shape, eps=1e-6):
    """[n0*n1*n2] bool: a coordinate within eps of a half-integer (rint is then decided by rounding noise)"""
    return R.tie_mask(as4x4(minv), native_shape, full_shape, eps)


def restore(x, minv, native_shape, full_shape, origin=(0, 0, 0), mode="nearest"):
    """x [C, d, h, w] on the box origin .. origin + (d, h, w) - 1 of the full grid -> float64 [C, n0, n1, n2]"""
    xn = np.asarray(x, dtype=np.float64)
    C, crop = xn.shape[0], np.asarray(xn.shape[1:])
    o = np.asarray(origin)
    s = coords(minv, native_shape, full_shape)
    r = np.rint(s).astype(int)
    inside = ((r >= o) & (r < o + crop)).all(1)
    if mode == "nearest":
        q = np.clip(r - o, 0, crop - 1)
        v = xn[:, q[:, 0], q[:, 1], q[:, 2]]
    else:
        f = np.floor(s)
        t = s - f
        lo = np.clip(f.astype(int) - o, 0, crop - 1)
        hi = np.clip(f.astype(int) + 1 - o, 0, crop - 1)
        v = 0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    iz, iy, ix = (hi if dz else lo)[:, 0], (hi if dy else lo)[:, 1], (hi if dx else lo)[:, 2]
                    w = (t[:, 0] if dz else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dx else 1 - t[:, 2])
                    v = v + w * xn[:, iz, iy, ix]
    return np.where(inside[None], v, 0.0).reshape(C, *(int(n) for n in native_shape))


def argmax_first(v):
    """[C, ...] -> [1, ...] uint8: the first maximal channel"""
    return np.argmax(v, 0)[None].astype(np.uint8)


def brats_label(ch):
    """the reference's plotting rule (unetr_segmentation_3d.py:95-101) on 4 boolean channels background / TC / WT / ET ->
    [1, ...] uint8: 1 where WT, then 2 where TC, then 3 where ET; a later rule overwrites an earlier one"""
    ch = np.asarray(ch).astype(bool)
    out = np.zeros(ch.shape[1:], dtype=np.uint8)
    out[ch[2]] = 1
    out[ch[1]] = 2
    out[ch[3]] = 3
    return out[None]


def discrete(v, inside, post):
    """the channels the BraTS rule sees: one-hot of the first-maximal argmax, or logit >= 0; background voxels have no channel set"""
    C = v.shape[0]
    m = np.asarray(inside).reshape(v.shape[1:])
    if post == "argmax":
        return (np.argmax(v, 0)[None] == np.arange(C).reshape(C, 1, 1, 1)) & m[None]
    return (v >= 0) & m[None]


def top_two_gap(v):
    """[...]: best minus second-best channel"""
    p = np.sort(v, 0)
    return p[-1] - p[-2]
