"""CPU restatements of the spacing-aware surface metrics (a helper module, not a test file), on top of metrics_ref.edges_ref
(MONAI 0.6.0's crop / squeeze / erosion edge rule) and its seeded cases.

(i)   directed_scipy: the distances of A's edge voxels to the nearest edge voxel of B by
      scipy.ndimage.distance_transform_edt(~edges_B, sampling=spacing) -- what a host MONAI / scipy evaluation does.
(ii)  directed_minplus: the same without scipy, as three float64 min-plus passes  f(i) = min_j g(j) + (s * (i - j))^2  in x, y,
      z order with +inf for "no edge" -- the form the kernels evaluate.
(iii) record_ref / hd_ref / asd_ref / nsd_ref: the reductions with np.percentile and np.mean and the nan / inf rules of
      DESIGN.md section 11.
"""
import math

import numpy as np
import torch

from metrics_ref import edges_ref


def pair_edges(pred, gt):
    """(edges_pred, edges_gt) bool numpy [ez,ey,ex] on the union box; two empty (0,0,0) arrays when both masks are empty"""
    ep, eg = edges_ref(pred.bool(), gt.bool())
    if ep is None:
        z = np.zeros((0, 0, 0), dtype=bool)
        return z, z
    return ep.numpy(), eg.numpy()


def directed_scipy(ea, eb, spacing):
    """float64 distances of the edge voxels ea to the nearest voxel of eb (C order of ea's voxels); all inf when eb is empty"""
    from scipy.ndimage import distance_transform_edt
    if not ea.any():
        return np.zeros(0)
    if not eb.any():
        return np.full(int(ea.sum()), np.inf)
    return np.asarray(distance_transform_edt(~eb, sampling=spacing)[ea], dtype=np.float64)


def sq_edt_minplus(feat, spacing):
    """float64 squared distance of every voxel to the nearest True voxel of feat (+inf where there is none)"""
    f = np.where(feat, 0.0, np.inf)
    for ax in (2, 1, 0):
        n = f.shape[ax]
        out = np.full_like(f, np.inf)
        shape = [1, 1, 1]
        shape[ax] = n
        i = np.arange(n)
        for j in range(n):
            t = spacing[ax] * (i - j).astype(np.float64)
            out = np.minimum(out, np.take(f, [j], axis=ax) + (t * t).reshape(shape))
        f = out
    return f


def directed_minplus(ea, eb, spacing):
    if not ea.any():
        return np.zeros(0)
    return np.sqrt(sq_edt_minplus(eb, spacing)[ea])


def _reduce(d, percentiles, tau):
    """max, mean, percentiles and the count within tau of one directed distance array"""
    if d.size == 0:
        return math.nan, math.nan, [math.nan] * len(percentiles), 0
    if np.isinf(d).all():                               # nothing to measure to: np.percentile of an all-inf array is nan
        return math.inf, math.inf, [math.nan] * len(percentiles), 0
    return float(d.max()), float(np.mean(d)), [float(np.percentile(d, q)) for q in percentiles], \
        (int((d <= tau).sum()) if tau is not None else 0)


def record_ref(pred, gt, spacing=(1.0, 1.0, 1.0), percentiles=(), tau=None, directed_fn=directed_scipy):
    """the fields of surface_metrics for one (pred, gt) pair of bool [D,H,W] masks, as Python numbers"""
    ep, eg = pair_edges(pred, gt)
    dpg, dgp = directed_fn(ep, eg, spacing), directed_fn(eg, ep, spacing)
    mx1, mean1, p1, w1 = _reduce(dpg, percentiles, tau)
    mx2, mean2, p2, w2 = _reduce(dgp, percentiles, tau)
    return dict(n_pred=float(dpg.size), n_gt=float(dgp.size), max_pg=mx1, max_gp=mx2, mean_pg=mean1, mean_gp=mean2,
                pct_pg=p1, pct_gp=p2, within_pg=float(w1), within_gp=float(w2), d_pg=dpg, d_gp=dgp)


def py_max(d1, d2):
    return d2 if d2 > d1 else d1                          # Python max(d1, d2) with nan: d1 unless d2 > d1


def hd_ref(rec, k=None, directed=False):
    """Hausdorff distance of a record: the max (k None) or its k-th percentile"""
    d1, d2 = (rec["max_pg"], rec["max_gp"]) if k is None else (rec["pct_pg"][k], rec["pct_gp"][k])
    return d1 if directed else py_max(d1, d2)


def asd_ref(rec, symmetric=False):
    return float(np.mean((rec["mean_pg"], rec["mean_gp"]))) if symmetric else rec["mean_pg"]


def nsd_ref(rec):
    n = rec["n_pred"] + rec["n_gt"]
    return (rec["within_pg"] + rec["within_gp"]) / n if n else math.nan


def batch_ref(preds, gts, fn):
    """[B, 1] float64 tensor of fn(pred, gt) over a list of pairs"""
    return torch.tensor([[fn(p, g)] for p, g in zip(preds, gts)], dtype=torch.float64)
