"""CPU restatement of RandCropAugment's random rotation and zoom (a helper module, not a test file; extends augment_ref).

These semantics are this project's own, not MONAI's RandAffined.  What is pinned here:

(i)   affine_words / draw_affine_row: Philox blocks 3 and 4 of a sample, the float32 angles and zooms, the matrix; replay_affine
      replays the device's ``aug.affine`` table.  Blocks 0..2 (augment_ref.sample_words) are not touched.
(ii)  build_matrix: M = R0 . R1 . R2 . diag(1/z) in double from the STORED float32 angles and zooms, rounded once to float32.
(iii) source_coords / affine_sample: the float32 coordinate map and the trilinear / nearest gather in the device's operation
      order, every step one torch float32 elementwise op (no lerp, no addcmul: nothing here can fuse a multiply and an add).
(iv)  apply_affine_ref: a whole batch from a params table and an affine table; unflagged rows go through augment_ref.apply_ref.
"""
import math
import struct

import numpy as np
import torch

import augment_ref as R

AFFINE_COLS = 16        # flag, 3 angles, 3 zooms, M row-major
F32 = torch.float32


# ---------------------------------------------------------------- (i) the draws
def affine_words(seed, call, s):
    """blocks 3 and 4 of sample s in call `call` (counter (call, s, j, 0), key (seed, 0)).
    Assignment:  block 3: [0] u < affine_prob flags the sample, [1..3] angle about spatial axis 0..2
                 block 4: [0..2] zoom of axis 0..2; zoom_per_axis=False uses [0] for all three"""
    return [R.philox4x64_10((call, s, j, 0), (seed, 0)) for j in (3, 4)]


def _uniform32(lo, hi, w):
    """lo + (hi - lo) * u in double, rounded to float32 (the stored value), as augment_ref draws the shift offset"""
    return float(np.float32(lo + (hi - lo) * R.u01(w)))


def _matmul3(a, b):
    """3x3 product in double, each entry (a0*b0 + a1*b1) + a2*b2"""
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def build_matrix(angles, zooms):
    """float32 [9], row-major: (R0 . R1) . R2 with column b scaled by 1 / z_b, in double from float32-valued angles and zooms.
    R2(t) = [[c, -s, 0], [s, c, 0], [0, 0, 1]] turns (q0, q1); R0 and R1 are its cyclic analogues (R0 turns (q1, q2), R1 (q2, q0))."""
    c, s = [math.cos(float(t)) for t in angles], [math.sin(float(t)) for t in angles]
    r0 = [[1.0, 0.0, 0.0], [0.0, c[0], -s[0]], [0.0, s[0], c[0]]]
    r1 = [[c[1], 0.0, s[1]], [0.0, 1.0, 0.0], [-s[1], 0.0, c[1]]]
    r2 = [[c[2], -s[2], 0.0], [s[2], c[2], 0.0], [0.0, 0.0, 1.0]]
    r = _matmul3(_matmul3(r0, r1), r2)
    inv = [1.0 / float(z) for z in zooms]
    return np.array([[r[a][b] * inv[b] for b in range(3)] for a in range(3)], dtype=np.float64).astype(np.float32).reshape(9)


IDENTITY_ROW = [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def draw_affine_row(cfg, seed, call, s):
    """the 16 float32 values of sample s: flag, angles, zooms, M"""
    b3, b4 = affine_words(seed, call, s)
    if not R.u01(b3[0]) < cfg["affine_prob"]:
        return list(IDENTITY_ROW)
    ang = [_uniform32(-r, r, b3[1 + a]) for a, r in enumerate(cfg["rotate_range"])]
    lo, hi = cfg["zoom_range"]
    zm = [_uniform32(lo, hi, b4[a if cfg["zoom_per_axis"] else 0]) for a in range(3)]
    return [1.0, *ang, *zm, *build_matrix(ang, zm).tolist()]


def affine_config(aug):
    return dict(R.aug_config(aug), affine_prob=aug.affine_prob, rotate_range=aug.rotate_range, zoom_range=aug.zoom_range,
                zoom_per_axis=aug.zoom_per_axis)


def replay_affine(cfg, ncalls, call=0):
    """the [B, 16] float32 tables of `ncalls` calls starting at device call counter `call`"""
    return [torch.tensor([draw_affine_row(cfg, cfg["seed"], call + n, s) for s in range(cfg["batch_size"])], dtype=F32)
            for n in range(ncalls)]


def affine_row(angles=(0.0, 0.0, 0.0), zooms=(1.0, 1.0, 1.0), matrix=None, flag=1.0):
    """a table row for apply(): M from the float32-rounded angles and zooms unless `matrix` (9 values, row-major) is given"""
    ang = [float(np.float32(t)) for t in angles]
    zm = [float(np.float32(z)) for z in zooms]
    m = build_matrix(ang, zm).tolist() if matrix is None else [float(np.float32(v)) for v in np.asarray(matrix).reshape(9)]
    return [float(flag), *ang, *zm, *m]


# ---------------------------------------------------------------- (iii) coordinates and the gather, float32, fixed order
def source_coords(S, corner, flips, k, axes, M, dims):
    """float32 [3, S0, S1, S2]: the source position of every output voxel, clamped to [-1, dim] per axis.
    p = crop position behind rot90^k and the flips (augment_ref.source_index with corner 0); q = p - (S - 1) / 2;
    src_a = (c0_a + (S_a - 1) / 2) + ((M[a][0] * q0 + M[a][1] * q1) + M[a][2] * q2)"""
    p = R.source_index(S, (0, 0, 0), flips, k, axes)
    m = torch.as_tensor(np.asarray(M, dtype=np.float32).reshape(3, 3))
    half = [torch.tensor(float(S[a] - 1), dtype=F32) * torch.tensor(0.5, dtype=F32) for a in range(3)]
    q = [p[a].to(F32) - half[a] for a in range(3)]
    out = []
    for a in range(3):
        centre = torch.tensor(float(corner[a]), dtype=F32) + half[a]
        dot = (m[a, 0] * q[0] + m[a, 1] * q[1]) + m[a, 2] * q[2]
        src = centre + dot
        out.append(torch.clamp(src, min=-1.0, max=float(np.float32(dims[a]))))
    return torch.stack(out)


def _taps(sc, dims):
    """per axis: i0, i1 (int64, clamped to the volume) and t (float32) of clamped coordinates sc [3, ...]"""
    i0, i1, t = [], [], []
    for a in range(3):
        f = torch.floor(sc[a])
        t.append(sc[a] - f)
        i0.append(f.long().clamp(0, dims[a] - 1))
        i1.append((f.long() + 1).clamp(0, dims[a] - 1))
    return i0, i1, t


def trilinear_f32(img, sc):
    """img [C, D, H, W] float32 at coordinates sc: lerp a + t * (b - a) along the last axis, then the middle, then the first"""
    i0, i1, t = _taps(sc, img.shape[1:])
    z, y, x = (i0[0], i1[0]), (i0[1], i1[1]), (i0[2], i1[2])

    def lerp(a, b, w):
        d = b - a
        return a + w * d

    plane = []
    for iz in range(2):
        row = [lerp(img[:, z[iz], y[iy], x[0]], img[:, z[iz], y[iy], x[1]], t[2]) for iy in range(2)]
        plane.append(lerp(row[0], row[1], t[1]))
    return lerp(plane[0], plane[1], t[0])


def nearest(lbl, sc):
    """lbl [L, D, H, W] at index floor(sc + 0.5) per axis, clamped to the volume"""
    idx = [torch.floor(sc[a] + torch.tensor(0.5, dtype=F32)).long().clamp(0, lbl.shape[1 + a] - 1) for a in range(3)]
    return lbl[:, idx[0], idx[1], idx[2]]


def affine_sample(img, lbl, corner, S, flips, k, axes, M):
    """one flagged sample before shift and normalize: x [C, *S] float32, y [L, *S] float32"""
    sc = source_coords(S, corner, flips, k, axes, M, img.shape[1:])
    return trilinear_f32(img, sc), nearest(lbl, sc).float()


# ---------------------------------------------------------------- (iv) a whole batch
def apply_affine_ref(images, labels, params, affine, S, axes=(0, 1), normalize=False):
    """x [B, C, *S], y [B, L, *S] from a params table [B, 8] and an affine table [B, 16]; per sample: the affine gather at crop
    time, flips, rot90, shift, normalize.  Rows with flag 0 are augment_ref.apply_ref's."""
    xs, ys = [], []
    for n, (r, a) in enumerate(zip(params.tolist(), affine.to(F32))):
        if float(a[0]) == 0.0:
            x, y = R.apply_ref(images, labels, params[n:n + 1], S, axes, normalize=normalize)
            xs.append(x[0])
            ys.append(y[0])
            continue
        vol, corner, flips, k, shift, bits = r[0], r[1:4], r[4], r[5], r[6], r[7]
        x, y = affine_sample(images[vol], labels[vol], corner, S, flips, k, axes, a[7:16].numpy())
        if shift:
            x = x + torch.tensor(struct.unpack("<f", struct.pack("<i", bits))[0], dtype=F32)
        if normalize:
            x = R.normalize_ref(x)
        xs.append(x)
        ys.append(y)
    return torch.stack(xs), torch.stack(ys)
