"""GPU time of class-balanced crop sampling (profiles/class_sampling.txt).

    python tools/bench_class_sampling.py [--rounds 7] [--calls 200] [--trace]

(1) VolumeCache.build_class_indices on one 512 x 512 x 300 volume with 14 classes (background and 13 boxes of very different
    sizes) against the torch route on the same GPU, [torch.nonzero(label.view(-1) == c) for c in range(14)]: host clock around
    work that ends in a synchronise, two warm-up rounds, then --rounds rounds alternating the two; every list is compared with
    torch.nonzero's.
    The fg / bg index lists of VolumeCache.add on the same volume: unetr_aug_index_count + unetr_aug_index_scatter back to back
    between two HIP events (add itself reads the two lengths back in between), the lists compared with the cache's.
(2) One aug(x, y) call at 8 x 96^3 with sampling="label_classes" against "pos_neg": HIP events around --calls calls, --rounds
    windows per mode, alternating.
--trace runs five builds and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/bench_class_sampling.py --trace`.
Needs a GPU: there is no CPU path.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, H, W, K = 300, 512, 512, 14


def make_cache(pkg, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    lbl = torch.zeros(1, D, H, W, device=dev)
    for c in range(1, K):
        sz = [max(4, int(s * (0.04 + 0.03 * (c % 5)))) for s in (D, H, W)]
        o = [int(torch.randint(0, s - z, (1,), generator=g, device=dev)) for s, z in zip((D, H, W), sz)]
        lbl[0, o[0]:o[0] + sz[0], o[1]:o[1] + sz[1], o[2]:o[2] + sz[2]] = c
    cache = pkg.VolumeCache(dev)
    cache.add(torch.rand(1, D, H, W, device=dev, generator=g), lbl)
    return cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_class_sampling needs a GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    dev = torch.device("cuda:0")
    cache = make_cache(pkg, dev)
    u8 = cache.label(0).view(-1)

    def build():
        cache._classes, cache._class_table = [], None           # drop the lists: the next call builds them again
        torch.cuda.synchronize()
        t = time.perf_counter()
        cache.build_class_indices(K)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def torch_route():
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = [torch.nonzero(u8 == c) for c in range(K)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    img, nfg, nbg = cache.image(0), cache.fg_indices(0).numel(), cache.bg_indices(0).numel()
    nws = pkg._capi.load().unetr_aug_index_ws_ints(u8.numel())
    ws = torch.empty(nws, dtype=torch.int32, device=dev)
    fg = torch.empty(max(nfg, 1), dtype=torch.int32, device=dev)
    bg = torch.empty(max(nbg, 1), dtype=torch.int32, device=dev)

    def index_lists():
        st = torch.cuda.current_stream().cuda_stream
        lists = (img.data_ptr(), u8.data_ptr(), 1, 1, u8.numel(), cache.image_threshold, ws.data_ptr(), nws)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pkg._capi.call("unetr_aug_index_count", *lists, st)
        pkg._capi.call("unetr_aug_index_scatter", *lists, fg.data_ptr(), bg.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if args.trace:
        for _ in range(5):
            build()
        return
    for _ in range(2):
        build()
        torch_route()
        index_lists()
    tb, tt, ti = [], [], []
    for _ in range(args.rounds):
        tb.append(build())
        ti.append(index_lists())
        ms, r = torch_route()
        tt.append(ms)
    equal = all(torch.equal(cache.class_indices(0, c).long(), r[c].view(-1)) for c in range(K))
    listed = sum(cache.class_counts(0))
    print(f"lists equal torch.nonzero: {equal}; class counts {cache.class_counts(0)}")
    print(f"voxels {u8.numel()}, listed {listed}: 2 label reads + 4 B per entry = {(2 * u8.numel() + 4 * listed) / 1e6:.1f} MB")
    same = torch.equal(fg[:nfg], cache.fg_indices(0)) and torch.equal(bg[:nbg], cache.bg_indices(0))
    print(f"index lists equal the cache's: {same}; fg {nfg}, bg {nbg}, ws total {ws[nws - 2:].tolist()}")
    for name, v in (("build_class_indices", tb), ("torch.nonzero x %d" % K, tt), ("index count + scatter", ti)):
        print(f"{name:22s} ms: median {statistics.median(v):.3f} min {min(v):.3f} max {max(v):.3f}")

    kw = dict(spatial_size=96, num_samples=4, batch_size=8, seed=1)
    augs = {"label_classes": pkg.RandCropAugment(cache, sampling="label_classes", num_classes=K, **kw),
            "pos_neg": pkg.RandCropAugment(cache, sampling="pos_neg", **kw)}
    x = torch.empty(8, 1, 96, 96, 96, device=dev)
    y = torch.empty(8, 1, 96, 96, 96, device=dev)
    for a in augs.values():
        for _ in range(20):
            a(x, y)
    torch.cuda.synchronize()
    res = {k: [] for k in augs}
    for _ in range(args.rounds):
        for k, a in augs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                a(x, y)
            e1.record()
            torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / args.calls * 1e3)
    for k, v in res.items():
        print(f"aug(x, y) 8 x 96^3 {k:13s} us per call: median {statistics.median(v):.2f} min {min(v):.2f} max {max(v):.2f}")


if __name__ == "__main__":
    main()
