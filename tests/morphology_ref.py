"""scipy references of the morphology module over [B, C, D, H, W] numpy arrays (every (item, channel) is its own mask, set
where != 0; results are uint8 0 / 1), and the project's pinned semantics of ``FillHoles`` restated with scipy.

The FillHoles rule (MONAI's fill_holes as the project pins it; MONAI 0.6.0 has no such transform to run): on a class-id map a
component of the background ``img == 0``, labelled with ``generate_binary_structure(3, connectivity)`` (None = 3), is filled
with label l when it touches none of the six faces, the set of non-zero values among the structure neighbours of its voxels is
exactly {l}, and l is in ``applied_labels`` (None = every label)."""
import numpy as np
from scipy import ndimage


def structure(connectivity):
    return ndimage.generate_binary_structure(3, connectivity)


def _planes(x, fn):
    x = np.asarray(x)
    out = np.empty(x.shape, np.uint8)
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            out[b, c] = fn(x[b, c] != 0)
    return out


def dilation(x, iterations=1, connectivity=1, border_value=0):
    return _planes(x, lambda m: ndimage.binary_dilation(m, structure(connectivity), iterations, border_value=border_value))


def erosion(x, iterations=1, connectivity=1, border_value=0):
    return _planes(x, lambda m: ndimage.binary_erosion(m, structure(connectivity), iterations, border_value=border_value))


def opening(x, iterations=1, connectivity=1):
    return _planes(x, lambda m: ndimage.binary_opening(m, structure(connectivity), iterations))


def closing(x, iterations=1, connectivity=1):
    return _planes(x, lambda m: ndimage.binary_closing(m, structure(connectivity), iterations))


def contour(x, connectivity=1):
    return _planes(x, lambda m: m & ~ndimage.binary_erosion(m, structure(connectivity)))


def fill_holes(x, connectivity=1):
    return _planes(x, lambda m: ndimage.binary_fill_holes(m, structure(connectivity)))


def face_labels(lab):
    """the labels that occur on the six faces of a 3-D label map"""
    faces = [lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]]
    return set(np.unique(np.concatenate([f.ravel() for f in faces])).tolist())


def fill_holes_restated(x, connectivity=1):
    """binary_fill_holes said the way the kernels compute it: the mask plus every component of its complement that touches no face"""
    def one(m):
        lab, n = ndimage.label(~m, structure(connectivity))
        holes = np.isin(lab, [l for l in range(1, n + 1) if l not in face_labels(lab)])
        return m | holes
    return _planes(x, one)


def fill_holes_rule(ids, applied_labels=None, connectivity=None):
    """the FillHoles rule on a class-id map [B, 1, D, H, W]; returns an array of the same dtype"""
    ids = np.asarray(ids)
    st = structure(3 if connectivity is None else connectivity)
    out = ids.copy()
    for b in range(ids.shape[0]):
        img = ids[b, 0]
        lab, n = ndimage.label(img == 0, st)
        on_face = face_labels(lab)
        boxes = ndimage.find_objects(lab)
        for l in range(1, n + 1):
            if l in on_face:
                continue
            box = tuple(slice(max(s.start - 1, 0), s.stop + 1) for s in boxes[l - 1])
            comp = lab[box] == l
            ring = ndimage.binary_dilation(comp, st) & ~comp
            around = set(np.unique(img[box][ring]).tolist()) - {0}
            if len(around) == 1:
                (v,) = around
                if applied_labels is None or v in applied_labels:
                    out[b, 0][box][comp] = v
    return out
