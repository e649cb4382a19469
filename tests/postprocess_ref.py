"""CPU references for the connected-component post-processing, on numpy arrays.

Two independent labellings of one plane of class words w [D, H, W] (0 = not labelled):
  label_plane_scipy   scipy.ndimage.label per class with generate_binary_structure(3, connectivity); canonical labels
                      (1 + smallest linear index of the component) from scipy.ndimage.minimum of the linear index
  label_plane_bfs     a literal breadth-first flood fill in raster order, for tiny volumes
and the semantics of the public functions on top of either: reference(...) returns (out, labels, sizes).
"""
from collections import deque

import numpy as np
from scipy import ndimage


def label_plane_scipy(w, connectivity):
    """(labels, sizes) int32 [D, H, W]"""
    w = np.asarray(w)
    lin = np.arange(w.size, dtype=np.int64).reshape(w.shape)
    labels = np.zeros(w.shape, np.int32)
    sizes = np.zeros(w.shape, np.int32)
    structure = ndimage.generate_binary_structure(3, connectivity)
    for k in np.unique(w[w != 0]):
        lab, n = ndimage.label(w == k, structure=structure)
        if n == 0:
            continue
        first = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, n + 1))).astype(np.int64)
        count = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        fg = lab > 0
        labels[fg] = (first[lab[fg] - 1] + 1).astype(np.int32)
        sizes[fg] = count[lab[fg] - 1].astype(np.int32)
    return labels, sizes


def _offsets(connectivity):
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < abs(dz) + abs(dy) + abs(dx) <= connectivity]


def label_plane_bfs(w, connectivity):
    """the same by flood fill: visiting seeds in raster order makes the seed the smallest linear index of its component"""
    w = np.asarray(w)
    D, H, W = w.shape
    labels = np.zeros(w.shape, np.int32)
    sizes = np.zeros(w.shape, np.int32)
    offs = _offsets(connectivity)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                if w[z, y, x] == 0 or labels[z, y, x]:
                    continue
                lab = (z * H + y) * W + x + 1
                labels[z, y, x] = lab
                members, queue = [(z, y, x)], deque([(z, y, x)])
                while queue:
                    cz, cy, cx = queue.popleft()
                    for dz, dy, dx in offs:
                        nz, ny, nx = cz + dz, cy + dy, cx + dx
                        if 0 <= nz < D and 0 <= ny < H and 0 <= nx < W and not labels[nz, ny, nx] \
                                and w[nz, ny, nx] == w[z, y, x]:
                            labels[nz, ny, nx] = lab
                            members.append((nz, ny, nx))
                            queue.append((nz, ny, nx))
                for m in members:
                    sizes[m] = len(members)
    return labels, sizes


def keep_plane(w, labels, sizes, rule, min_size):
    """bool [D, H, W]: voxels that survive.  rule 0: per class word the component with the most voxels, the smallest label
    among equals (= argmax(bincount(labels)[1:]) over raster-ordered labels); rule 1: components of at least min_size voxels"""
    keep = np.asarray(w) == 0
    if rule == 1:
        return keep | (sizes >= min_size)
    for k in np.unique(w[w != 0]):
        lab_k = labels[w == k]
        uniq, count = np.unique(lab_k, return_counts=True)      # ascending labels = raster order of the first voxel
        keep |= (w == k) & (labels == uniq[np.argmax(count)])
    return keep


def argmax_first(logits):
    """first-maximum argmax over the channel axis as float32 class ids [B, 1, D, H, W]"""
    return np.argmax(logits, axis=1)[:, None].astype(np.float32)


def reference(x, connectivity=None, applied_labels=None, independent=True, from_logits=False, rule=0, min_size=0,
              labeller=label_plane_scipy):
    """(out, labels, sizes) with the layouts of the package's functions"""
    conn = 3 if connectivity is None else connectivity
    x = np.asarray(x, np.float32)
    if from_logits:
        C = x.shape[1]
        x = argmax_first(x)
        if applied_labels is None:
            applied_labels = list(range(1, C))
    B, C = x.shape[:2]
    out = x.copy()
    labels = np.zeros(x.shape, np.int32)
    sizes = np.zeros(x.shape, np.int32)
    if C == 1:
        ids = list(range(1, 32)) if applied_labels is None else list(np.atleast_1d(applied_labels))
        for b in range(B):
            m = x[b, 0]
            applied = np.isin(m, ids)
            w = np.where(applied, m if independent else 1, 0).astype(np.int64)
            lab, sz = labeller(w, conn)
            labels[b, 0], sizes[b, 0] = lab, sz
            out[b, 0] = np.where(keep_plane(w, lab, sz, rule, min_size), m, 0)
        return out, labels, sizes
    chans = list(range(C)) if applied_labels is None else list(np.atleast_1d(applied_labels))
    for b in range(B):
        if independent:
            for c in chans:
                w = (x[b, c] != 0).astype(np.int64)
                lab, sz = labeller(w, conn)
                labels[b, c], sizes[b, c] = lab, sz
                out[b, c] = np.where(keep_plane(w, lab, sz, rule, min_size), x[b, c], 0)
        else:
            w = np.any(x[b, chans] != 0, axis=0).astype(np.int64)
            lab, sz = labeller(w, conn)
            keep = keep_plane(w, lab, sz, rule, min_size)
            for c in chans:
                on = x[b, c] != 0
                labels[b, c], sizes[b, c] = np.where(on, lab, 0), np.where(on, sz, 0)
                out[b, c] = np.where(keep, x[b, c], 0)
    return out, labels, sizes
