"""CPU restatements of the validation metrics (a helper module, not a test file).

(i)   hd_torch: torch only, no scipy -- MONAI 0.6.0's crop / squeeze / erosion edge rule and an exact squared EDT as three
      brute-force min-plus passes  f(i) = min_j g(j) + (i - j)^2,  np.percentile's linear rule restated.
(ii)  hd_monai_scipy: a literal restatement of the recalled MONAI 0.6.0 code path (get_mask_edges, get_surface_distance,
      compute_percent_hausdorff_distance, compute_hausdorff_distance) on scipy.ndimage.
(iii) confusion_matrix_ref / cm_metric_ref / reduction_ref: get_confusion_matrix, compute_confusion_matrix_metric and
      do_metric_reduction.
"""
import math

import numpy as np
import torch

INF_SQ = 1 << 40


# ---------------------------------------------------------------- (i) torch-only Hausdorff distance
def edges_ref(pred: torch.Tensor, gt: torch.Tensor):
    """edge masks of two bool [D,H,W] masks on the bounding box of pred | gt (None, None when both are empty) and the box"""
    union = pred | gt
    if not bool(union.any()):
        return None, None
    idx = union.nonzero()
    lo, hi = idx.min(0).values.tolist(), (idx.max(0).values + 1).tolist()
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    out = []
    for m in (pred[sl], gt[sl]):
        er = m.clone()
        for ax in range(3):
            if m.shape[ax] == 1:                       # np.squeeze drops the axis: no erosion along it
                continue
            p = torch.nn.functional.pad(m.to(torch.uint8), pad=_pad_axis(ax), value=0).bool()   # border value 0
            n = m.shape[ax]
            er &= p.narrow(ax, 0, n) & p.narrow(ax, 2, n)
        out.append(m & ~er)
    return out[0], out[1]


def _pad_axis(ax):
    pad = [0] * 6
    k = (2 - ax) * 2
    pad[k], pad[k + 1] = 1, 1
    return pad


def sq_edt_ref(feat: torch.Tensor) -> torch.Tensor:
    """exact squared distance (int64) of every voxel to the nearest True voxel of feat [D,H,W] (>= INF_SQ where none)"""
    f = torch.where(feat, torch.zeros((), dtype=torch.int64), torch.full((), INF_SQ, dtype=torch.int64))
    for ax in range(3):
        n = f.shape[ax]
        i = torch.arange(n)
        out = torch.full_like(f, INF_SQ)
        shape = [1, 1, 1]
        shape[ax] = n
        for j in range(n):
            d = ((i - j) ** 2).view(shape)
            out = torch.minimum(out, f.narrow(ax, j, 1) + d)
        f = out.clamp_max(INF_SQ)
    return f


def np_percentile_ref(sorted_vals, n, q):
    """np.percentile(values, q * 100) (method 'linear', NumPy 2.x) of n ascending float64 values given as a callable k -> value"""
    vi = (n - 1) * q
    if vi >= n - 1:
        prev = nxt = n - 1
        gamma = vi + 1.0                              # numpy indexes -1 there
    else:
        prev = math.floor(vi)
        nxt = prev + 1
        gamma = vi - prev
    a, b = sorted_vals(prev), sorted_vals(nxt)
    diff = b - a
    if gamma >= 0.5:
        return b - diff * (1.0 - gamma)
    return a + diff * gamma


def _directed_ref(ea, eb, percentile):
    if ea is None or not bool(ea.any()):
        return math.nan
    if not bool(eb.any()):
        return math.nan if percentile else math.inf
    d2 = sq_edt_ref(eb)[ea]
    if not percentile:
        return math.sqrt(float(d2.max()))
    s = torch.sort(d2).values
    return np_percentile_ref(lambda k: math.sqrt(float(s[k])), s.numel(), float(percentile) / 100.0)


def hd_pair_ref(pred, gt, percentile=None, directed=False):
    ep, eg = edges_ref(pred.bool(), gt.bool())
    d1 = _directed_ref(ep, eg, percentile)
    if directed:
        return d1
    d2 = _directed_ref(eg, ep, percentile)
    return max(d1, d2)                                # Python max, as MONAI: d1 unless d2 > d1


def hd_torch(y_pred, y, include_background=False, percentile=None, directed=False):
    """[B, C] float64 Hausdorff distance of one-hot [B,C,D,H,W] tensors (mask = value == 1)"""
    y_pred, y = y_pred.cpu(), y.cpu()
    if not include_background:
        y_pred, y = y_pred[:, 1:], y[:, 1:]
    B, C = y_pred.shape[:2]
    out = torch.empty(B, C, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            out[b, c] = hd_pair_ref(y_pred[b, c] == 1, y[b, c] == 1, percentile, directed)
    return out


# ---------------------------------------------------------------- (ii) the recalled MONAI 0.6.0 code path on scipy
def _get_mask_edges(seg_pred, seg_gt, label_idx=1):
    from scipy.ndimage import binary_erosion
    if seg_pred.dtype != bool:
        seg_pred = seg_pred == label_idx
    if seg_gt.dtype != bool:
        seg_gt = seg_gt == label_idx
    if not np.any(seg_pred | seg_gt):
        return np.zeros_like(seg_pred), np.zeros_like(seg_gt)
    union = seg_pred | seg_gt
    nz = np.nonzero(union)
    sl = tuple(slice(int(a.min()), int(a.max()) + 1) for a in nz)
    seg_pred, seg_gt = np.squeeze(seg_pred[sl]), np.squeeze(seg_gt[sl])
    edges_pred = binary_erosion(seg_pred) ^ seg_pred
    edges_gt = binary_erosion(seg_gt) ^ seg_gt
    return edges_pred, edges_gt


def _get_surface_distance(seg_pred, seg_gt):
    from scipy.ndimage import distance_transform_edt
    if not np.any(seg_gt):
        dis = np.inf * np.ones_like(seg_gt)
    else:
        dis = distance_transform_edt(~seg_gt)
    return np.asarray(dis[seg_pred])


def _compute_percent_hd(edges_pred, edges_gt, percentile):
    surface_distance = _get_surface_distance(edges_pred, edges_gt)
    if surface_distance.shape == (0,):
        return np.nan
    if not percentile:
        return surface_distance.max()
    return np.percentile(surface_distance, percentile)


def hd_monai_scipy(y_pred, y, include_background=False, percentile=None, directed=False):
    y_pred, y = y_pred.detach().cpu().float().numpy(), y.detach().cpu().float().numpy()
    if not include_background:
        y_pred, y = y_pred[:, 1:], y[:, 1:]
    B, C = y_pred.shape[:2]
    hd = np.empty((B, C))
    for b, c in np.ndindex(B, C):
        edges_pred, edges_gt = _get_mask_edges(y_pred[b, c], y[b, c])
        d1 = _compute_percent_hd(edges_pred, edges_gt, percentile)
        if directed:
            hd[b, c] = d1
        else:
            d2 = _compute_percent_hd(edges_gt, edges_pred, percentile)
            hd[b, c] = max(d1, d2)
    return torch.from_numpy(hd)


# ---------------------------------------------------------------- (iii) confusion matrix and reduction
def confusion_matrix_ref(y_pred, y, include_background=True):
    """[B, C, 4] float64 (tp, fp, tn, fn) of binarised [B,C,...] tensors"""
    y_pred, y = y_pred.detach().cpu().double(), y.detach().cpu().double()
    if not include_background:
        y_pred, y = y_pred[:, 1:], y[:, 1:]
    B, C = y_pred.shape[:2]
    p, t = y_pred.reshape(B, C, -1), y.reshape(B, C, -1)
    V = p.shape[-1]
    tp = (p * t).sum(-1)
    fp = p.sum(-1) - tp
    fn = t.sum(-1) - tp
    tn = V - tp - fp - fn
    return torch.stack([tp, fp, tn, fn], -1)


CM_FORMULAS = {
    "tpr": lambda tp, fp, tn, fn: (tp, tp + fn),
    "tnr": lambda tp, fp, tn, fn: (tn, fp + tn),
    "ppv": lambda tp, fp, tn, fn: (tp, tp + fp),
    "npv": lambda tp, fp, tn, fn: (tn, tn + fn),
    "fnr": lambda tp, fp, tn, fn: (fn, tp + fn),
    "fpr": lambda tp, fp, tn, fn: (fp, fp + tn),
    "fdr": lambda tp, fp, tn, fn: (fp, fp + tp),
    "for": lambda tp, fp, tn, fn: (fn, fn + tn),
    "ts": lambda tp, fp, tn, fn: (tp, tp + fn + fp),
    "acc": lambda tp, fp, tn, fn: (tp + tn, tp + fn + fp + tn),
    "f1": lambda tp, fp, tn, fn: (tp * 2.0, tp * 2.0 + fn + fp),
}
CM_ALIASES = {
    "tpr": ["sensitivity", "recall", "hit_rate", "true_positive_rate", "tpr", "Hit Rate", "TRUE_POSITIVE_RATE"],
    "tnr": ["specificity", "tnr"],
    "ppv": ["precision", "ppv", "Precision"],
    "npv": ["npv"],
    "fnr": ["miss_rate", "fnr", "miss rate"],
    "fpr": ["fall_out", "fpr", "Fall Out"],
    "fdr": ["fdr"],
    "for": ["for"],
    "ts": ["threat_score", "csi", "threat score"],
    "acc": ["accuracy"],
    "f1": ["f1_score", "F1 Score"],
}


def cm_metric_ref(key, cm):
    tp, fp, tn, fn = (cm[..., k] for k in range(4))
    num, den = CM_FORMULAS[key](tp, fp, tn, fn)
    return torch.where(den != 0, num / den, torch.full_like(num, math.nan))


def reduction_ref(f, reduction):
    """do_metric_reduction: nan-ignoring mean over classes then items ("mean") or over items per class ("mean_batch"),
    written with explicit loops"""
    f = f.double()
    if reduction == "mean_batch":
        out = []
        for c in range(f.shape[1]):
            out.append(_nanmean0(f[:, c]))
        return torch.stack(out).reshape(f.shape[1:])
    per_item = torch.stack([_nanmean0(f[b]) for b in range(f.shape[0])])
    has = torch.stack([(~torch.isnan(f[b])).any(0) for b in range(f.shape[0])])
    cnt = has.double().sum(0)
    s = torch.where(has, per_item, torch.zeros_like(per_item)).sum(0)
    return torch.where(cnt > 0, s / cnt.clamp_min(1), torch.zeros(1, dtype=s.dtype))   # MONAI's t_zero: at least 1-d


def _nanmean0(x):
    """mean over dim 0 ignoring NaN (0 where all are NaN); an inf propagates"""
    ok = ~torch.isnan(x)
    s = torch.where(ok, x, torch.zeros_like(x)).sum(0)
    n = ok.double().sum(0)
    return torch.where(n > 0, s / n.clamp_min(1), torch.zeros_like(s))


# ---------------------------------------------------------------- seeded cases shared by the CPU and GPU tests
def _blob(shape, center, radii):
    zz, yy, xx = torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in shape], indexing="ij")
    return ((zz - center[0]) / radii[0]) ** 2 + ((yy - center[1]) / radii[1]) ** 2 + ((xx - center[2]) / radii[2]) ** 2 <= 1.0


def hd_edge_cases(shape=(11, 10, 9)):
    """(name, pred, gt) bool [D,H,W] masks: empty, single voxel, 1-thick plates and lines, objects on the volume faces"""
    D, H, W = shape
    z = lambda: torch.zeros(shape, dtype=torch.bool)
    cases = []
    blob = _blob(shape, (5, 4, 4), (3, 2.5, 3))
    cases += [("empty_pred", z(), blob), ("empty_gt", blob, z()), ("both_empty", z(), z())]
    one = z(); one[4, 5, 6] = True
    cases += [("single_voxel_both", one, one.clone()), ("single_voxel_vs_blob", one, blob)]
    two = z(); two[4, 5, 2] = True
    cases += [("two_single_voxels", one, two)]
    plate = z(); plate[3, 2:5, 3:6] = True                 # 1 x 3 x 3 plate: extent 1 along z
    plate2 = z(); plate2[3, 1:7, 2:8] = True
    cases += [("plate_3x3", plate, plate.clone()), ("plates", plate, plate2)]
    line = z(); line[2, 4, 1:8] = True                     # extent 1 along z and y
    line2 = z(); line2[2, 4, 3:5] = True
    cases += [("line", line, line2), ("line_vs_blob", line, blob)]
    colz = z(); colz[:, 3, 3] = True                       # a column through the whole volume (touches two faces)
    cases += [("column", colz, blob)]
    face = z(); face[:, :, 0:2] = True                     # slab on the x = 0 face
    full = torch.ones(shape, dtype=torch.bool)
    cases += [("face_slab", face, blob), ("full_vs_blob", full, blob), ("full_vs_full", full, full.clone())]
    corner = z(); corner[D - 3:, H - 3:, W - 3:] = True
    cases += [("corner", corner, face)]
    return cases


def hd_random_cases(n, shape=(11, 10, 9), seed=0):
    """n seeded pairs of random blobs (union of ellipsoids plus speckle)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        masks = []
        for _ in range(2):
            m = torch.zeros(shape, dtype=torch.bool)
            for _ in range(int(torch.randint(1, 4, (1,), generator=g))):
                c = [float(torch.randint(0, s, (1,), generator=g)) for s in shape]
                r = [0.5 + 3.0 * float(torch.rand(1, generator=g)) for _ in shape]
                m |= _blob(shape, c, r)
            m |= torch.rand(shape, generator=g) > 0.97
            masks.append(m)
        out.append((f"random_{k}", masks[0], masks[1]))
    return out


def as_onehot(pred, gt):
    """[1, 2, D, H, W] float one-hot pair (channel 0 = complement, channel 1 = the mask)"""
    p = torch.stack([~pred, pred]).float()[None]
    t = torch.stack([~gt, gt]).float()[None]
    return p, t
