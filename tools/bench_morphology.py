"""GPU time of the bit-packed binary morphology and the hole filling.

    python tools/bench_morphology.py [--iters 20] [--no-cpu]

Prints ONE JSON line.  Input: the one-hot ellipsoid "organs" of tools/bench_metrics.py at [1,14,160,160,128] float32 with 1 % of
the voxels flipped (speckle and pinholes).  Per workload the median of --iters warmed calls timed with HIP events:

    closing2     binary_closing(iterations=2), connectivity 1 (the default) and 3
    dilation5    binary_dilation(iterations=5, connectivity=3); also iterations 1 and 8 (what a launch of 4 fused steps costs
                 beside pack + unpack) and the same from uint8
    fill_holes   binary_fill_holes (connectivity 1), and the connected_components call inside it alone

against two baselines:

    torch   the same operation from torch.nn.functional.max_pool3d on the same GPU.  A 3x3x3 max pool is the dilation by the
            full cube, so this covers connectivity 3 only; erosion is 1 - pool(1 - x) with the complement padded by ones
            (border_value 0).  Five 3x3x3 pools and one 11x11x11 pool are both timed for dilation5.  Hole filling has no
            pooling form (it needs the components of the complement), so it has no torch row.
    scipy   scipy.ndimage on the host per channel, including the device -> host -> device copies, run once (skipped by --no-cpu)
"""
import argparse
import importlib
import json
import time

import torch
import torch.nn.functional as F

from bench_metrics import onehot, synthetic_organs, time_gpu

SHAPE = (1, 14, 160, 160, 128)


def pool_dilate(x, n):
    for _ in range(n):
        x = F.max_pool3d(x, 3, 1, 1)
    return x


def pool_erode(x, n):
    x = 1 - x
    for _ in range(n):
        x = F.max_pool3d(F.pad(x, (1,) * 6, value=1.0), 3, 1, 0)
    return 1 - x


def via_scipy(x, fn):
    """fn per channel on the host, timed from the device tensor to the device result"""
    import numpy as np
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = x.cpu().numpy() != 0
    out = np.stack([np.stack([fn(m[b, c]) for c in range(m.shape[1])]) for b in range(m.shape[0])])
    res = torch.from_numpy(out.astype("float32")).to(x.device)
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the scipy baseline")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_morphology: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    dev = torch.device("cuda:0")
    B, C, D, H, W = SHAPE
    _, labels = synthetic_organs(B, C, D, H, W, seed=7, device=dev)
    x = onehot(labels, C)
    flip = torch.rand(x.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(8)) < 0.01
    x = torch.where(flip, 1 - x, x).contiguous()
    x8 = x.to(torch.uint8)
    t = lambda fn: time_gpu(fn, a.iters)
    out = {"iters": a.iters, "shape": list(SHAPE), "foreground": float(x.mean())}

    out["closing2"] = {
        "c1_ms": t(lambda: pkg.binary_closing(x, iterations=2)),
        "c3_ms": t(lambda: pkg.binary_closing(x, iterations=2, connectivity=3)),
        "torch_c3_ms": t(lambda: pool_erode(pool_dilate(x, 2), 2)),
        "equals_torch_c3": bool(torch.equal(pkg.binary_closing(x, iterations=2, connectivity=3), pool_erode(pool_dilate(x, 2), 2)))}
    out["dilation5"] = {
        "c3_ms": t(lambda: pkg.binary_dilation(x, iterations=5, connectivity=3)),
        "c3_uint8_ms": t(lambda: pkg.binary_dilation(x8, iterations=5, connectivity=3)),
        "c3_1_iteration_ms": t(lambda: pkg.binary_dilation(x, iterations=1, connectivity=3)),
        "c3_8_iterations_ms": t(lambda: pkg.binary_dilation(x, iterations=8, connectivity=3)),
        "torch_c3_5_pools_ms": t(lambda: pool_dilate(x, 5)),
        "torch_c3_1_pool_11_ms": t(lambda: F.max_pool3d(x, 11, 1, 5)),
        "equals_torch_c3": bool(torch.equal(pkg.binary_dilation(x, iterations=5, connectivity=3), pool_dilate(x, 5)))}
    out["fill_holes"] = {
        "c1_ms": t(lambda: pkg.binary_fill_holes(x)),
        "labelling_alone_ms": t(lambda: pkg.connected_components((x == 0).to(torch.float32), 1)),
        "filled_voxels": int((pkg.binary_fill_holes(x) - x).sum())}
    if not a.no_cpu:
        from scipy import ndimage
        st = ndimage.generate_binary_structure
        for key, ours, fn in (
                ("closing2", lambda: pkg.binary_closing(x, iterations=2), lambda m: ndimage.binary_closing(m, st(3, 1), 2)),
                ("dilation5", lambda: pkg.binary_dilation(x, iterations=5, connectivity=3), lambda m: ndimage.binary_dilation(m, st(3, 3), 5)),
                ("fill_holes", lambda: pkg.binary_fill_holes(x), lambda m: ndimage.binary_fill_holes(m))):
            ref, secs = via_scipy(x, fn)
            out[key]["scipy_with_copies_s"] = secs
            out[key]["equals_scipy"] = bool(torch.equal(ours(), ref))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
