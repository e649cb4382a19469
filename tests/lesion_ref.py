"""CPU references for the instance-level metrics, on numpy arrays, one plane [D, H, W] at a time.

  lesion_loop       the definition of record: the literal per-lesion loop -- per lesion a dilation, np.unique of the predicted
                    labels under it, np.isin, Dice
  lesion_pairs      the restatement the kernels implement: ONE dilation and ONE labelling of the whole ground truth, the table of
                    the distinct (lesion, component) pairs, per-label accumulators
  panoptic_brute    panoptic quality by brute force over all pairs of components
  PairTableModel    a model of the kernels' open-addressing insertion: same hash, same probing, same capacity
Both lesion forms return the same record (``finish``); sums of float terms are math.fsum, i.e. correctly rounded.
"""
import functools
import math

import numpy as np
from scipy import ndimage

M64 = (1 << 64) - 1


def canonical_labels(mask, connectivity):
    """int64 [D, H, W]: 1 + the smallest linear index of the voxel's component, 0 outside the mask"""
    mask = np.asarray(mask) != 0
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, connectivity))
    out = np.zeros(mask.shape, np.int64)
    if n:
        lin = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
        first = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, n + 1))).astype(np.int64)
        out[mask] = first[lab[mask] - 1] + 1
    return out


def dilate(mask, iterations, connectivity):
    if iterations == 0:
        return np.asarray(mask) != 0
    return ndimage.binary_dilation(np.asarray(mask) != 0, ndimage.generate_binary_structure(3, connectivity), iterations=iterations)


def finish(n_gt, n_pred, dice, n_fn, n_fp, n_tp_pred):
    """the record of a plane from its per-lesion Dice values (matched, not ignored lesions; ascending lesion label)"""
    n_tp = len(dice)
    nan = float("nan")
    dice_sum = math.fsum(dice)
    den = n_tp + n_fn + n_fp
    precision = n_tp_pred / (n_tp_pred + n_fp) if n_tp_pred + n_fp else nan
    recall = n_tp / (n_tp + n_fn) if n_tp + n_fn else nan
    if math.isnan(precision) or math.isnan(recall):
        f1 = nan
    else:
        f1 = 2.0 * precision * recall / (precision + recall) if precision + recall else 0.0
    return dict(n_gt=n_gt, n_tp=n_tp, n_fn=n_fn, n_fp=n_fp, n_pred=n_pred, n_tp_pred=n_tp_pred, dice=list(dice), dice_sum=dice_sum,
                lesion_dice=dice_sum / den if den else 1.0, precision=precision, recall=recall, f1=f1)


def lesion_loop(pred, gt, dilation=3, dilation_connectivity=2, connectivity=3, min_lesion_voxels=0):
    """the literal loop.  Lesions: the ground-truth voxels under each component of the dilated ground truth (components whose
    dilations touch are one lesion), visited in raster order of the dilated component's first voxel."""
    pred, gt = np.asarray(pred) != 0, np.asarray(gt) != 0
    structure = ndimage.generate_binary_structure(3, connectivity)
    dil_lab, n_gt = ndimage.label(dilate(gt, dilation, dilation_connectivity), structure=structure)
    gt_lab = dil_lab * gt
    pred_lab, n_pred = ndimage.label(pred, structure=structure)
    dice, n_fn = [], 0
    matched_any, matched_counted = set(), set()
    for i in range(1, n_gt + 1):
        lesion = gt_lab == i
        under = dilate(lesion, dilation, dilation_connectivity)
        matched = np.unique(pred_lab[under])
        matched = matched[matched != 0]
        matched_any.update(matched.tolist())
        gv = int(lesion.sum())
        if gv < min_lesion_voxels:
            continue
        if matched.size == 0:
            n_fn += 1
            continue
        matched_counted.update(matched.tolist())
        pm = np.isin(pred_lab, matched)
        dice.append(2 * int((lesion & pm).sum()) / (int(pm.sum()) + gv))
    return finish(n_gt, n_pred, dice, n_fn, n_pred - len(matched_any), len(matched_counted))


def pair_dict(a, b, mask=None):
    """{(a, b): [voxels, masked voxels]} over the voxels where both labels are non-zero"""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    m = np.ones(a.shape, bool) if mask is None else np.asarray(mask).ravel() != 0
    on = (a != 0) & (b != 0)
    table = {}
    for x, y, w in zip(a[on].tolist(), b[on].tolist(), m[on].tolist()):
        e = table.setdefault((x, y), [0, 0])
        e[0] += 1
        e[1] += int(w)
    return table


def lesion_pairs(pred, gt, dilation=3, dilation_connectivity=2, connectivity=3, min_lesion_voxels=0):
    """the same record from the pair table of (DL, PL): DL labels the dilation of the WHOLE ground truth, PL the prediction"""
    pred, gt = np.asarray(pred) != 0, np.asarray(gt) != 0
    DL = canonical_labels(dilate(gt, dilation, dilation_connectivity), connectivity)
    PL = canonical_labels(pred, connectivity)
    gv = dict(zip(*[v.tolist() for v in np.unique(DL[gt], return_counts=True)]))
    size_p = dict(zip(*[v.tolist() for v in np.unique(PL[pred], return_counts=True)]))
    pv, inter, flag = {}, {}, {}
    for (i, p), (_, nm) in pair_dict(DL, PL, gt).items():
        pv[i] = pv.get(i, 0) + size_p[p]
        inter[i] = inter.get(i, 0) + nm
        flag[p] = flag.get(p, 0) | (3 if gv[i] >= min_lesion_voxels else 1)
    dice, n_fn = [], 0
    for i in sorted(gv):
        if gv[i] < min_lesion_voxels:
            continue
        if i in pv:
            dice.append(2 * inter[i] / (pv[i] + gv[i]))
        else:
            n_fn += 1
    return finish(len(gv), len(size_p), dice, n_fn, len(size_p) - len(flag), sum(1 for f in flag.values() if f & 2))


def panoptic_brute(pred, gt, connectivity=3):
    """tp / fp / fn, sq, rq, pq over ALL pairs of a ground-truth and a predicted component; IoU > 1/2 decided in integers"""
    GL, PL = canonical_labels(gt, connectivity), canonical_labels(pred, connectivity)
    ga, gb = np.unique(GL[GL != 0]), np.unique(PL[PL != 0])
    ious = []
    for i in ga.tolist():
        A = GL == i
        sa = int(A.sum())
        for j in gb.tolist():
            Bm = PL == j
            n = int((A & Bm).sum())
            u = sa + int(Bm.sum()) - n
            if 2 * n > u:
                ious.append(n / u)
    tp = len(ious)
    fp, fn = len(gb) - tp, len(ga) - tp
    nan = float("nan")
    if len(ga) + len(gb) == 0:
        return dict(tp=0, fp=0, fn=0, iou=[], sq=nan, rq=nan, pq=nan)
    sq = math.fsum(ious) / tp if tp else 0.0
    rq = tp / (tp + 0.5 * fp + 0.5 * fn)
    return dict(tp=tp, fp=fp, fn=fn, iou=ious, sq=sq, rq=rq, pq=sq * rq)


# ---- the open-addressing table of csrc/lesion.hip

def table_slots(max_pairs):
    s = 2
    while s < 2 * max_pairs:
        s <<= 1
    return s


def hash64(k):
    """the finalizer of MurmurHash3 on a 64-bit key"""
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def pack(a, b):
    return (int(a) << 32) | int(b)


class PairTableModel:
    """slots = 2 * max_pairs rounded up to a power of two, key 0 = empty, linear probing bounded by the slots, a full table
    drops the pair; ``pairs`` counts the claimed slots and ``overflow`` is pairs > max_pairs"""

    def __init__(self, max_pairs):
        self.max_pairs = max_pairs
        self.slots = table_slots(max_pairs)
        self.keys = np.zeros(self.slots, np.uint64)
        self.vals = np.zeros((self.slots, 2), np.int64)
        self.pairs = 0

    def insert(self, key, n, nm=0):
        s = hash64(key) & (self.slots - 1)
        for _ in range(self.slots):
            if self.keys[s] == 0:
                self.keys[s] = key
                self.pairs += 1
            if int(self.keys[s]) == key:
                self.vals[s] += (n, nm)
                return True
            s = (s + 1) & (self.slots - 1)
        return False

    @property
    def overflow(self):
        return self.pairs > self.max_pairs

    def as_dict(self):
        return table_as_dict(self.keys, self.vals)


def table_as_dict(keys, vals):
    """{(a, b): [voxels, masked voxels]} of the occupied slots"""
    return {(int(k) >> 32, int(k) & 0xffffffff): [int(v[0]), int(v[1])] for k, v in zip(keys, vals) if int(k) != 0}


def probe_chains_closed(keys):
    """every occupied slot is reachable from its key's home slot through occupied slots only (the invariant of linear probing
    without deletion, whatever the insertion order): ties the hash of a table read back from the device to ``hash64``"""
    slots = len(keys)
    for s, k in enumerate(keys):
        if int(k) == 0:
            continue
        h = hash64(int(k)) & (slots - 1)
        while h != s:
            if int(keys[h]) == 0:
                return False
            h = (h + 1) & (slots - 1)
    return True


# ---- test volumes

def blobs(shape, n, rng, max_extent=(3, 3, 4)):
    m = np.zeros(shape, np.uint8)
    for _ in range(n):
        e = [int(rng.integers(1, k + 1)) for k in max_extent]
        o = [int(rng.integers(0, max(1, s - k + 1))) for s, k in zip(shape, e)]
        m[o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]] = 1
    return m


def lesion_case(shape, seed, n_gt=5, n_spurious=3):
    """(pred, gt) uint8 [D, H, W]: gt = a few boxes; pred = gt shifted by one voxel along x with some boxes dropped, plus
    spurious boxes"""
    rng = np.random.default_rng(seed)
    gt = blobs(shape, n_gt, rng)
    lab, n = ndimage.label(gt)
    keep = np.concatenate([[False], rng.random(n) < 0.7])
    pred = np.roll(keep[lab].astype(np.uint8), 1, axis=2)
    pred[:, :, 0] = 0
    return np.maximum(pred, blobs(shape, n_spurious, rng, (2, 2, 2))), gt


@functools.lru_cache(maxsize=None)
def picked_planes(shape, dilation, min_lesion_voxels=0, dilation_connectivity=2, connectivity=3):
    """(pred, gt, records) for a batch shape [B, C, D, H, W]: per plane the first seed whose reference (the literal loop) has at
    least two lesions, a matched one and an unmatched prediction among them"""
    B, C = shape[:2]
    pred, gt = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    records = []
    seed = 0
    for b in range(B):
        for c in range(C):
            while True:
                seed += 1
                p, g = lesion_case(shape[2:], seed)
                r = lesion_loop(p, g, dilation, dilation_connectivity, connectivity, min_lesion_voxels)
                if r["n_gt"] >= 2 and r["n_fp"] >= 1 and r["n_tp"] >= 1:
                    break
                assert seed < 2000, "no seed gives an informative plane"
            pred[b, c], gt[b, c] = p, g
            records.append(r)
    return pred, gt, records
