"""GPU time of one RandCropAugment call (sampler + gather [+ normalize]).

    python tools/bench_augment.py [--iters 50] [--cpu] [--no-intensity | --trace-intensity]

Prints ONE JSON line: per case the median of --iters warmed calls timed with HIP events, the same with every sample rotated
(rot90_prob=1) and unrotated (rot90_prob=0), the bytes the call must move and the implied rate.  With --cpu also the wall time
of the CPU restatement (tests/augment_ref.py::apply_ref) on the same params, run once.  Each case is also timed with every
sample rotated and zoomed (affine_prob=1, rotate_range 30 degrees about each axis, zoom_range (0.7, 1.4): "affine_us"), with
the bytes that gather must move at the least -- the distinct source voxels under the warped footprints of its last call
(image taps 4 B x C, label voxels 1 B x L) plus the bytes written -- its floor at 8 TB/s, the achieved rate, the ratio to the
plain call and the share of the 4.3 ms training step.  Cases:
  ct: 1 item x 4 samples of 96^3 from a 1-channel 320x320x200 volume, 14 classes, scale + foreground crop, all transforms
  mr: 1 item x 4 samples of 128^3 from a 4-channel 240x240x155 volume, 3 label channels, all transforms + normalize
Intensity augmentation (unless --no-intensity): the same call with intensity=IntensityAugment.nnunet() ("intensity_nnunet_us")
and with every probability 1 ("intensity_all_us"); for the latter the bytes its five passes must move on top of the plain call
(intensity_pass_bytes), the floor of the whole call at 8 TB/s, and the time of an eager-torch restatement of the five
operations alone on the same x (F.conv3d blur, torch.randn noise, amin / amax / mean, pow; applied to every sample, since eager
code cannot branch per sample without a host sync), to be compared with intensity_all_us - us.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def synthetic_volume(C, L, shape, ncls, seed, device):
    """CT-like intensities (body sphere ~100 HU on -200 HU air) and ncls - 1 spherical organs (L = 1) or L nested shells"""
    g = torch.Generator(device=device).manual_seed(seed)
    zz, yy, xx = torch.meshgrid(*[torch.linspace(-1, 1, s, device=device) for s in shape], indexing="ij")
    r = (zz ** 2 + yy ** 2 + xx ** 2).sqrt()
    img = torch.randn(C, *shape, generator=g, device=device) * 50 + 300 * (r < 0.9).float() - 200
    if L == 1:
        lbl = torch.zeros(1, *shape, device=device)
        for c in range(1, ncls):
            cz, cy, cx = (torch.rand(3, generator=g, device=device) * 1.2 - 0.6).tolist()
            lbl[0][((zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2).sqrt() < 0.08 + 0.02 * (c % 4)] = c
    else:
        lbl = torch.stack([(r < 0.2 + 0.1 * c).float() for c in range(L)])
    return img, lbl


def time_calls(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def affine_floor_bytes(aug, cache, C, L, normalize):
    """the least bytes the affine call just made must move: distinct source voxels of every sample's footprint + the output"""
    import augment_affine_ref as A
    dims = cache.shapes[0][2:]
    S = aug.spatial_size
    src = 0
    for r, a in zip(aug.params.cpu().tolist(), aug.affine.cpu()):
        if float(a[0]) == 0.0:
            src += S[0] * S[1] * S[2] * (C * 4 + L)
            continue
        sc = A.source_coords(S, r[1:4], r[4], r[5], aug.spatial_axes, a[7:16].numpy(), dims)
        i0, i1, _ = A._taps(sc, dims)
        taps = torch.zeros(dims, dtype=torch.bool)
        for z in (i0[0], i1[0]):
            for y in (i0[1], i1[1]):
                for x in (i0[2], i1[2]):
                    taps[z, y, x] = True
        near = torch.zeros(dims, dtype=torch.bool)
        n = [torch.floor(sc[k] + 0.5).long().clamp(0, dims[k] - 1) for k in range(3)]
        near[n[0], n[1], n[2]] = True
        src += int(taps.sum()) * C * 4 + int(near.sum()) * L
    nvox = aug.batch_size * S[0] * S[1] * S[2]
    return src + nvox * (C + L) * 4 + (2 * nvox * C * 4 if normalize else 0)


def intensity_pass_bytes(nvox_c):
    """bytes the intensity passes move for nvox_c = B * C * V float32 voxels with every operation flagged: three blur passes,
    noise / brightness / statistics, contrast / gamma, each one read and one write"""
    return 4 * nvox_c * 2 * 5


def torch_intensity(x, sigma=0.75, std=0.05, brightness=1.1, contrast=1.1, gamma=1.2):
    """the five operations in eager torch on every sample of x [B, C, S, S, S] (mid-range values); returns the result"""
    import torch.nn.functional as F
    R = int(max(4.0 * sigma, 0.5) + 0.5)
    k = torch.arange(-R, R + 1, device=x.device, dtype=torch.float32)
    w = torch.exp(-(k * k) / (2.0 * sigma * sigma))
    w = w / w.sum()
    v = x.reshape(-1, 1, *x.shape[2:])
    for a in range(3):
        shape, pad = [1, 1, 1, 1, 1], [0] * 6
        shape[2 + a] = 2 * R + 1
        pad[2 * (2 - a)] = pad[2 * (2 - a) + 1] = R
        v = F.conv3d(F.pad(v, pad, mode="replicate"), w.view(shape))
    v = v.reshape(x.shape)
    v = v + std * torch.randn_like(v)
    v = v * brightness
    dims = (2, 3, 4)
    mn, mx, mean = v.amin(dims, keepdim=True), v.amax(dims, keepdim=True), v.mean(dims, keepdim=True)
    v = torch.minimum(torch.maximum((v - mean) * contrast + mean, mn), mx)
    mn, mx = v.amin(dims, keepdim=True), v.amax(dims, keepdim=True)
    rng = mx - mn
    return ((v - mn) / (rng + 1e-7)).pow(gamma) * rng + mn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-intensity", action="store_true", help="skip the intensity cases (A/B runs of the plain call)")
    ap.add_argument("--trace-intensity", action="store_true",
                    help="only the every-probability-1 call of each case: the run to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--cpu", action="store_true", help="also time the CPU restatement once per case")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    dev = torch.device("cuda:0")
    cases = {
        "ct": dict(C=1, L=1, shape=(320, 320, 200), ncls=14, add=dict(scale_range=(-175, 250, 0.0, 1.0), crop_foreground=True),
                   aug=dict(spatial_size=96, num_samples=4, normalize=None)),
        "mr": dict(C=4, L=3, shape=(240, 240, 155), ncls=0, add=dict(),
                   aug=dict(spatial_size=128, num_samples=4, normalize="nonzero_channel_wise")),
    }
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    for name, c in cases.items():
        img, lbl = synthetic_volume(c["C"], c["L"], c["shape"], c["ncls"], seed=0, device=dev)
        cache = pkg.VolumeCache(dev)
        t0 = time.perf_counter()
        cache.add(img, lbl, **c["add"])
        torch.cuda.synchronize()
        add_ms = (time.perf_counter() - t0) * 1e3
        del img, lbl
        res = {"add_ms_first_call": round(add_ms, 2), "volume": list(cache.shapes[0])}
        S = c["aug"]["spatial_size"]
        B = c["aug"]["num_samples"]
        x = torch.empty(B, c["C"], S, S, S, device=dev)
        y = torch.empty(B, c["L"], S, S, S, device=dev)
        if args.trace_intensity:
            full = pkg.IntensityAugment(noise_prob=1.0, blur_prob=1.0, brightness_prob=1.0, contrast_prob=1.0, gamma_prob=1.0)
            aug = pkg.RandCropAugment(cache, pos=1, neg=1, flip_prob=(0.1, 0.1, 0.1), rot90_prob=0.1, max_k=3, shift_offsets=0.1,
                                      shift_prob=0.5, seed=1, intensity=full, **c["aug"])
            out[name] = {"intensity_all_us": round(time_calls(lambda: aug(x, y), args.iters), 2)}
            continue
        for label, rot in (("us", 0.1), ("us_rot0", 0.0), ("us_rot1", 1.0)):
            aug = pkg.RandCropAugment(cache, pos=1, neg=1, flip_prob=(0.1, 0.1, 0.1), rot90_prob=rot, max_k=3, shift_offsets=0.1,
                                      shift_prob=0.5, seed=1, **c["aug"])
            res[label] = round(time_calls(lambda: aug(x, y), args.iters), 2)
        nvox = B * S ** 3
        moved = nvox * (c["C"] * 4 + c["L"]) + nvox * (c["C"] + c["L"]) * 4
        if c["aug"]["normalize"]:
            moved += 2 * nvox * c["C"] * 4
        res["bytes_moved"] = moved
        res["GBps"] = round(moved / (res["us"] * 1e-6) / 1e9, 1)
        aug = pkg.RandCropAugment(cache, pos=1, neg=1, flip_prob=(0.1, 0.1, 0.1), rot90_prob=0.1, max_k=3, shift_offsets=0.1,
                                  shift_prob=0.5, seed=1, affine_prob=1.0, rotate_range=0.5236, zoom_range=(0.7, 1.4), **c["aug"])
        res["affine_us"] = round(time_calls(lambda: aug(x, y), args.iters), 2)
        floor = affine_floor_bytes(aug, cache, c["C"], c["L"], c["aug"]["normalize"])
        res["affine_bytes_floor"] = floor
        res["affine_floor_us_at_8TBps"] = round(floor / 8e12 * 1e6, 2)
        res["affine_GBps"] = round(floor / (res["affine_us"] * 1e-6) / 1e9, 1)
        res["affine_over_plain"] = round(res["affine_us"] / res["us"], 2)
        res["affine_share_of_4.3ms_step"] = round(res["affine_us"] / 4300.0, 4)
        if not args.no_intensity:
            full = pkg.IntensityAugment(noise_prob=1.0, blur_prob=1.0, brightness_prob=1.0, contrast_prob=1.0, gamma_prob=1.0)
            for label, it in (("intensity_nnunet_us", pkg.IntensityAugment.nnunet()), ("intensity_all_us", full)):
                aug = pkg.RandCropAugment(cache, pos=1, neg=1, flip_prob=(0.1, 0.1, 0.1), rot90_prob=0.1, max_k=3, shift_offsets=0.1,
                                          shift_prob=0.5, seed=1, intensity=it, **c["aug"])
                res[label] = round(time_calls(lambda: aug(x, y), args.iters), 2)
            extra = intensity_pass_bytes(nvox * c["C"])
            res["intensity_pass_bytes"] = extra
            res["intensity_all_floor_us_at_8TBps"] = round((moved + extra) / 8e12 * 1e6, 2)
            res["intensity_all_minus_plain_us"] = round(res["intensity_all_us"] - res["us"], 2)
            res["intensity_passes_GBps"] = round(extra / (res["intensity_all_minus_plain_us"] * 1e-6) / 1e9, 1)
            res["intensity_all_share_of_4.3ms_step"] = round(res["intensity_all_us"] / 4300.0, 4)
            try:
                res["torch_intensity_us"] = round(time_calls(lambda: torch_intensity(x), max(args.iters // 5, 5)), 2)
                res["torch_over_hip_passes"] = round(res["torch_intensity_us"] / res["intensity_all_minus_plain_us"], 1)
            except RuntimeError as e:                          # an eager comparison that cannot run is reported, not hidden
                res["torch_intensity_error"] = str(e).splitlines()[0][:200]
        if args.cpu:
            import augment_ref as R
            p = aug.params.cpu()
            t0 = time.perf_counter()
            R.apply_ref([cache.image(0)[0].cpu()], [cache.label(0)[0].cpu()], p, aug.spatial_size,
                        normalize=c["aug"]["normalize"] is not None)
            res["cpu_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out[name] = res
        del cache, aug, x, y
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
