"""GPU time of lesion_wise_metrics against the route users have today: copy both masks to the host and run the per-lesion loop
there.

    python tools/bench_lesion_metrics.py [--reps 5] [--size 155 240 240] [--no-kernels]

Prints ONE JSON line.  Two seeded pairs of masks (default volume 155x240x240, the BraTS grid):
  brats3       [1, 3, D, H, W]: about 20 ellipsoid lesions per channel; the prediction moves and rescales each one, misses a few
               and adds a few spurious components
  many_small   [1, 1, D, H, W]: 400 boxes of a few voxels each (some hundred lesions once near ones merge); the prediction shifts
               most of them by a voxel, misses the rest and adds 100 spurious boxes
Per input, two routes are timed around WHOLE calls after a warm-up, alternated in one process, --reps repetitions each, reported
as median and [min, max] in ms:
  gpu    lesion_wise_metrics(pred, gt, include_background=True), HIP events
  host   pred.cpu(), gt.cpu() -> the loop of the definition (per lesion a dilation, np.unique of the predicted labels under it,
         the matched components' voxels, Dice), wall clock.  The loop is the definition's, restricted to each lesion's bounding
         box grown by the dilation and with the matched components' sizes taken from one bincount: the fastest form that keeps
         its semantics, so the comparison errs towards the host.
and the results are compared (`equal`: integers equal, floats within 2 n^2 2^-53).  Unless --no-kernels, one further call per
input runs under torch.profiler; every kernel's device time is reported with its share of the call, and for the lo_* kernels the
bytes they must move per plane (V voxels, S table slots) and the implied rate against the 8 TB/s of HBM:
  insert    12 V          both label maps and the mask read (atomics only where both labels are set)
  fold      16 S          the table read; dense accumulators touched at the present pairs only
  clear     16 S + 20 V   tables and dense arrays written
  reduce    8 V           sizeA and sizeB read; the accumulators only at the labels that exist
  finalize  8 * partials
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BPS = 8e12
INTS = ("n_gt", "n_tp", "n_fn", "n_fp", "n_pred")
FLOATS = ("dice_sum", "lesion_dice", "precision", "recall", "f1")


def ellipsoid(m, c, r):
    lo = [max(0, int(math.floor(ci - ri))) for ci, ri in zip(c, r)]
    hi = [min(n, int(math.ceil(ci + ri)) + 1) for ci, ri, n in zip(c, r, m.shape)]
    z, y, x = np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij", sparse=True)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0


def make_inputs(size):
    rng = np.random.default_rng(0)
    size = tuple(size)
    gt, pred = np.zeros((1, 3) + size, bool), np.zeros((1, 3) + size, bool)
    for c in range(3):
        for k in range(20):
            ctr = rng.uniform(0.08, 0.92, 3) * size
            r = rng.uniform(2.0, 14.0, 3)
            ellipsoid(gt[0, c], ctr, r)
            if k % 7 != 6:                                           # three of twenty are missed
                ellipsoid(pred[0, c], ctr + rng.uniform(-2, 2, 3), r * rng.uniform(0.8, 1.2))
        for _ in range(5):
            ellipsoid(pred[0, c], rng.uniform(0.05, 0.95, 3) * size, rng.uniform(1.0, 4.0, 3))
    small_gt, small_pred = np.zeros((1, 1) + size, bool), np.zeros((1, 1) + size, bool)
    for k in range(500):
        o = [int(rng.integers(2, n - 6)) for n in size]
        e = rng.integers(1, 5, 3)
        box = (0, 0, slice(o[0], o[0] + e[0]), slice(o[1], o[1] + e[1]), slice(o[2], o[2] + e[2]))
        if k < 400:
            small_gt[box] = True
            if k % 10 < 7:
                small_pred[0, 0, o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2] + 1:o[2] + e[2] + 1] = True
        else:
            small_pred[box] = True
    return {"brats3": (pred, gt), "many_small": (small_pred, small_gt)}


def host_plane(pred, gt, dilation=3, dilation_connectivity=2, connectivity=3, min_lesion_voxels=0):
    """the per-lesion loop of DESIGN.md section 24 on one plane (bool [D, H, W]); returns the plane's record"""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, connectivity)
    ball = ndimage.generate_binary_structure(3, dilation_connectivity)
    grown = ndimage.binary_dilation(gt, ball, iterations=dilation) if dilation else gt
    dil_lab, n_gt = ndimage.label(grown, structure=structure)
    gt_lab = dil_lab * gt
    pred_lab, n_pred = ndimage.label(pred, structure=structure)
    size_p = np.bincount(pred_lab.ravel(), minlength=n_pred + 1)
    dice, n_fn = [], 0
    matched_any, matched_counted = set(), set()
    for i, box in enumerate(ndimage.find_objects(gt_lab, max_label=n_gt), start=1):
        box = tuple(slice(max(0, s.start - dilation), min(n, s.stop + dilation)) for s, n in zip(box, gt.shape))
        lesion = gt_lab[box] == i
        under = ndimage.binary_dilation(lesion, ball, iterations=dilation) if dilation else lesion
        plab = pred_lab[box]
        matched = np.unique(plab[under])
        matched = matched[matched != 0]
        matched_any.update(matched.tolist())
        gv = int(lesion.sum())
        if gv < min_lesion_voxels:
            continue
        if matched.size == 0:
            n_fn += 1
            continue
        matched_counted.update(matched.tolist())
        inter = int((lesion & np.isin(plab, matched)).sum())
        dice.append(2 * inter / (int(size_p[matched].sum()) + gv))
    n_tp, n_fp, n_tpp = len(dice), n_pred - len(matched_any), len(matched_counted)
    nan = float("nan")
    dice_sum = math.fsum(dice)
    den = n_tp + n_fn + n_fp
    precision = n_tpp / (n_tpp + n_fp) if n_tpp + n_fp else nan
    recall = n_tp / (n_tp + n_fn) if n_tp + n_fn else nan
    if math.isnan(precision) or math.isnan(recall):
        f1 = nan
    else:
        f1 = 2.0 * precision * recall / (precision + recall) if precision + recall else 0.0
    return dict(n_gt=n_gt, n_tp=n_tp, n_fn=n_fn, n_fp=n_fp, n_pred=n_pred, dice_sum=dice_sum,
                lesion_dice=dice_sum / den if den else 1.0, precision=precision, recall=recall, f1=f1)


def host_route(pred, gt):
    p, g = pred.cpu().numpy() != 0, gt.cpu().numpy() != 0
    return [host_plane(p[b, c], g[b, c]) for b in range(p.shape[0]) for c in range(p.shape[1])]


def equal(r, records):
    C = r.n_gt.shape[1]
    for i, rec in enumerate(records):
        b, c = divmod(i, C)
        if int(r.overflow[b, c]) or any(int(getattr(r, k)[b, c]) != rec[k] for k in INTS):
            return False
        for k in FLOATS:
            got, want = float(getattr(r, k)[b, c]), rec[k]
            if math.isnan(want) != math.isnan(got) or (not math.isnan(want) and abs(got - want) > 2 * rec["n_gt"] ** 2 * 2.0 ** -53):
                return False
    return True


def timed_gpu(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_host(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def kernel_times(fn):
    """device time in us of every kernel of one call, by name"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    times = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        t = float(e.cuda_time_total if t is None else t)
        if t > 0:
            name = e.key.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split()[-1].split("::")[-1]
            times[name] = times.get(name, 0.0) + t
    if not any(k.startswith("lo_insert") for k in times):
        raise SystemExit(f"bench_lesion_metrics: the profiler did not see the lo_* kernels, only {sorted(times)}")
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[155, 240, 240])
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lesion_metrics: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    dev = torch.device("cuda:0")
    V = args.size[0] * args.size[1] * args.size[2]
    S = pkg.lesion_metrics.table_slots(65536)
    out = {"device": torch.cuda.get_device_name(0), "volume": args.size, "reps": args.reps, "inputs": {}}
    for name, (pred, gt) in make_inputs(args.size).items():
        p, g = torch.from_numpy(pred).to(torch.float32).to(dev), torch.from_numpy(gt).to(torch.float32).to(dev)
        planes = p.shape[0] * p.shape[1]
        gpu = lambda: pkg.lesion_wise_metrics(p, g, include_background=True)
        host = lambda: host_route(p, g)
        r, records = gpu(), host()                                   # warms both routes
        res = {"planes": planes, "lesions": [rec["n_gt"] for rec in records], "predicted": [rec["n_pred"] for rec in records],
               "tp_fn_fp": [[rec["n_tp"], rec["n_fn"], rec["n_fp"]] for rec in records],
               "lesion_dice": [round(rec["lesion_dice"], 6) for rec in records], "equal": equal(r, records)}
        times = {"gpu": [], "host": []}
        for _ in range(args.reps):
            times["gpu"].append(timed_gpu(gpu))
            times["host"].append(timed_host(host))
        res.update({k: summary(v) for k, v in times.items()})
        res["speedup_gpu_vs_host"] = round(statistics.median(times["host"]) / statistics.median(times["gpu"]), 1)
        res["gpu_ahead_by_more_than_the_spread"] = max(times["gpu"]) < min(times["host"])
        if not args.no_kernels:
            kt = kernel_times(gpu)
            total = sum(kt.values())
            need = {"lo_insert_kernel": 12 * V * planes, "lo_fold_kernel": 16 * S * planes, "lo_reduce_kernel": 8 * V * planes,
                    "lo_clear_kernel": (16 * S + 20 * V) * planes}
            res["kernels_total_us"] = round(total, 1)
            res["kernels"] = {}
            for kname, us in sorted(kt.items(), key=lambda kv: -kv[1]):
                row = {"us": round(us, 1), "share": round(us / total, 4)}
                if kname in need:
                    row.update(bytes=need[kname], TBps=round(need[kname] / (us * 1e-6) / 1e12, 3),
                               fraction_of_8TBps=round(need[kname] / (us * 1e-6) / HBM_BPS, 4))
                res["kernels"][kname] = row
        out["inputs"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
