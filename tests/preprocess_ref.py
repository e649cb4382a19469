"""CPU restatement (float64) of the per-volume front of the reference's transform chain, MONAI 0.6.0 / nibabel semantics as
remembered from their sources (not pinned against their output):

    Spacing(pixdim, diagonal=False, mode, padding_mode="border", align_corners=False) -> Orientation(axcodes)

Two routes to the same result:
  library route   spacing_grid_sample (zoom_affine, compute_shape_offset, to_norm_affine, affine_grid + grid_sample with
                  reverse_indexing) followed by orientation (io_orientation, ornt_transform, flip / transpose)
  fused route     fused_gather: out[j] = interp(in, clamp(T @ M @ [j, 1], 0, shape - 1)), the formula csrc/preprocess.hip implements
"""
import numpy as np
import torch
import torch.nn.functional as F

AXCODE_LABELS = (("L", "R"), ("P", "A"), ("I", "S"))


# ---------------------------------------------------------------- Spacing
def zoom_affine(affine, scale):
    """monai.data.utils.zoom_affine(diagonal=False): the columns rescaled to length `scale`, rotation and shear kept"""
    affine = np.asarray(affine, dtype=np.float64)
    norm = np.sqrt(np.sum(np.square(affine), 0))[:-1]
    return affine @ np.diag(np.append(np.asarray(scale, dtype=np.float64) / norm, 1.0))


def compute_shape_offset(shape, in_affine, out_affine):
    """monai.data.utils.compute_shape_offset; the offset is the same-orientation branch (zoom_affine keeps the orientation)"""
    sr = len(shape)
    corners = np.asarray(np.meshgrid(*[(0.0, d - 1.0) for d in shape], indexing="ij")).reshape(sr, -1)
    corners = np.concatenate((corners, np.ones_like(corners[:1])))
    corners = in_affine @ corners
    out = np.linalg.inv(out_affine) @ corners
    out = out[:-1] / out[-1]
    out_shape = np.round(np.ptp(out, axis=1) + 1.0).astype(int)
    offset = in_affine @ np.array([0.0] * sr + [1.0])
    return out_shape, offset[:-1] / offset[-1]


def to_norm_affine_matrix(shape):
    """index -> normalised [-1, 1] coordinate of grid_sample with align_corners=False"""
    n = np.asarray(shape, dtype=np.float64)
    m = np.diag(np.append(2.0 / n, 1.0))
    m[:-1, -1] = 1.0 / n - 1.0
    return m


def spacing_transform(shape, affine, pixdim):
    """(new affine, output shape, T = inv(A) @ A_new, identity shortcut taken?)"""
    affine = np.asarray(affine, dtype=np.float64)
    new_affine = zoom_affine(affine, pixdim)
    out_shape, offset = compute_shape_offset(shape, affine, new_affine)
    new_affine[:3, -1] = offset
    T = np.linalg.inv(affine) @ new_affine
    if np.allclose(T, np.eye(4), atol=1e-3):
        return new_affine, np.asarray(shape), np.eye(4), True
    return new_affine, out_shape, T, False


def spacing_grid_sample(x, affine, pixdim, mode):
    """Spacing by the library's own composition; x [C, d0, d1, d2] (any dtype) -> float64 tensor, new affine, T"""
    shape = tuple(x.shape[1:])
    new_affine, out_shape, T, identity = spacing_transform(shape, affine, pixdim)
    x = torch.as_tensor(x).double()
    if identity:
        return x.clone(), new_affine, T
    theta = to_norm_affine_matrix(shape) @ T @ np.linalg.inv(to_norm_affine_matrix(out_shape))
    rev = [2, 1, 0, 3]                                   # reverse_indexing: grid_sample wants (x, y, z) = (d2, d1, d0)
    theta = theta[rev][:, rev]
    grid = F.affine_grid(torch.as_tensor(theta[:3])[None], [1, x.shape[0], *out_shape.tolist()], align_corners=False)
    out = F.grid_sample(x[None], grid, mode=mode, padding_mode="border", align_corners=False)[0]
    return out, new_affine, T


# ---------------------------------------------------------------- Orientation
def io_orientation(affine):
    """nibabel.orientations.io_orientation"""
    rzs = np.asarray(affine, dtype=np.float64)[:3, :3]
    zooms = np.sqrt((rzs * rzs).sum(0))
    zooms[zooms == 0] = 1
    rs = rzs / zooms
    P, S, Qs = np.linalg.svd(rs, full_matrices=False)
    tol = S.max() * 3 * np.finfo(S.dtype).eps
    keep = S > tol
    R = P[:, keep] @ Qs[keep]
    ornt = np.full((3, 2), np.nan)
    for i in range(3):
        col = R[:, i]
        if not np.allclose(col, 0):
            a = np.argmax(np.abs(col))
            ornt[i] = (a, -1 if col[a] < 0 else 1)
            R[a, :] = 0
    return ornt


def axcodes2ornt(axcodes):
    ornt = np.full((3, 2), np.nan)
    for i, code in enumerate(axcodes):
        for a, (lo, hi) in enumerate(AXCODE_LABELS):
            if code in (lo, hi):
                ornt[i] = (a, -1 if code == lo else 1)
    return ornt


def ornt_transform(start, end):
    out = np.full((3, 2), np.nan)
    for e_in, (e_out, e_flip) in enumerate(end):
        for s_in, (s_out, s_flip) in enumerate(start):
            if e_out == s_out:
                out[s_in] = (e_in, s_flip * e_flip)
    return out


def orientation(x, affine, axcodes="RAS"):
    """nibabel apply_orientation on the spatial axes of x [C, ...] (numpy) -> reoriented array, new affine, index map M (4x4:
    in_idx = M @ out_idx)"""
    t = ornt_transform(io_orientation(affine), axcodes2ornt(axcodes))
    shape = x.shape[1:]
    M = np.zeros((4, 4))
    M[3, 3] = 1
    y = x
    for i in range(3):
        a, f = int(t[i, 0]), t[i, 1]
        if f < 0:
            y = np.flip(y, i + 1)
            M[i, a], M[i, 3] = -1, shape[i] - 1
        else:
            M[i, a] = 1
    y = np.transpose(y, [0] + [int(p) + 1 for p in np.argsort(t[:, 0])])
    return np.ascontiguousarray(y), np.asarray(affine, dtype=np.float64) @ M, M


# ---------------------------------------------------------------- both routes
def library_route(x, affine, pixdim=(1.0, 1.0, 1.0), axcodes="RAS", mode="bilinear"):
    """Spacing -> Orientation as the library composes them: (float64 numpy [C, D, H, W], new affine, 4x4 T @ M)"""
    out, new_affine, T = spacing_grid_sample(x, affine, pixdim, mode)
    y, aff2, M = orientation(out.numpy(), new_affine, axcodes)
    return y, aff2, T @ M


def source_coords(matrix, out_shape, in_shape):
    """float64 source coordinates [D*H*W, 3] of every output voxel, clamped to the source (border padding)"""
    D, H, W = (int(s) for s in out_shape)
    j = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    s = j @ matrix[:3, :3].T + matrix[:3, 3]
    return np.clip(s, 0, np.asarray(in_shape, dtype=np.float64) - 1.0)


def fused_gather(x, matrix, out_shape, mode):
    """out[j] = interp(x, clamp(matrix @ [j, 1])) in float64; nearest rounds half to even (torch's nearbyint)"""
    xn = np.asarray(x, dtype=np.float64)
    C = xn.shape[0]
    D, H, W = (int(s) for s in out_shape)
    lim = np.asarray(xn.shape[1:]) - 1
    s = source_coords(matrix, out_shape, xn.shape[1:])
    if mode == "nearest":
        r = np.rint(s).astype(int)
        return xn[:, r[:, 0], r[:, 1], r[:, 2]].reshape(C, D, H, W)
    f = np.floor(s)
    t = s - f
    f = f.astype(int)
    c = np.minimum(f + 1, lim)
    out = 0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                iz, iy, ix = (c if dz else f)[:, 0], (c if dy else f)[:, 1], (c if dx else f)[:, 2]
                w = (t[:, 0] if dz else 1 - t[:, 0]) * (t[:, 1] if dy else 1 - t[:, 1]) * (t[:, 2] if dx else 1 - t[:, 2])
                out = out + w * xn[:, iz, iy, ix]
    return out.reshape(C, D, H, W)


def tie_mask(matrix, out_shape, in_shape, eps=1e-6):
    """[D*H*W] bool: a source coordinate within eps of a half-integer on some axis (nearest is then decided by rounding noise)"""
    s = source_coords(matrix, out_shape, in_shape)
    return (np.abs(s - np.floor(s) - 0.5) < eps).any(1)


def brats_channels(label):
    """ConvertToMultiChannelBasedOnBratsClassesd (unetr_segmentation_3d.py:65-93) on a [d0, d1, d2] label"""
    label = np.asarray(label)
    tc = np.logical_or(label == 2, label == 3)
    return np.stack([label == 0, tc, np.logical_or(tc, label == 1), label == 3], 0).astype(np.float32)


# ---------------------------------------------------------------- test inputs
def signed_permutation_affines(spacing, origin, angle):
    """the 48 affines whose axes are a signed permutation of `spacing`-scaled world axes, rotated by `angle` rad about z"""
    import itertools
    ca, sa = np.cos(angle), np.sin(angle)
    R = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            A = np.zeros((4, 4))
            A[3, 3] = 1
            for i in range(3):
                A[perm[i], i] = signs[i] * spacing[i]
            A[:3, :3] = R @ A[:3, :3]
            A[:3, 3] = origin
            out.append(A)
    return out
