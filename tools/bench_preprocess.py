"""GPU time of one preprocess.resample_orient call (Spacingd -> Orientationd [-> BraTS converter]).

    python tools/bench_preprocess.py [--iters 20] [--cpu]

Prints ONE JSON line: per case the median of --iters warmed kernel launches timed with HIP events (us; call_us is the whole
Python call with the host plan and the allocations), the bytes the kernel must move (source once + output once) and the
implied rate, and the same resampling done with torch on the same GPU (fp32, image only): torch.nn.functional.affine_grid +
grid_sample followed by flip / permute().contiguous(); where Spacing is the identity torch does the flip /
permute().contiguous() alone, as MONAI would.  With --cpu also the wall time of the float64 CPU restatement
(tests/preprocess_ref.py::library_route, image and label), run once.  Cases:
  ct: 1 x 512x512x90 int16 at (0.79, 0.79, 5.0) mm, LPS, to 1 mm RAS, with a one-channel label
  mr: 4 x 240x240x155 float32 at 1 mm, LPS to RAS (identity spacing: a pure reorientation), label through the BraTS converter
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def time_calls(fn, iters):
    for _ in range(3):
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


def torch_route(R, image, affine, pixdim):
    """the yardstick: returns a closure that resamples `image` [C, d0, d1, d2] with torch ops only (fp32)"""
    shape = tuple(image.shape[1:])
    new_affine, out_shape, T, identity = R.spacing_transform(shape, affine, pixdim)
    t = R.ornt_transform(R.io_orientation(new_affine), R.axcodes2ornt("RAS"))
    flips = [i + 1 for i in range(3) if t[i, 1] < 0]
    perm = [0] + [int(p) + 1 for p in np.argsort(t[:, 0])]
    theta = None
    if not identity:
        th = R.to_norm_affine_matrix(shape) @ T @ np.linalg.inv(R.to_norm_affine_matrix(out_shape))
        rev = [2, 1, 0, 3]
        theta = torch.as_tensor(th[rev][:, rev][:3], dtype=torch.float32, device=image.device)[None]
    size = [1, image.shape[0], *(int(s) for s in out_shape)]

    def run():
        x = image.float()
        if theta is not None:
            grid = F.affine_grid(theta, size, align_corners=False)
            x = F.grid_sample(x[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0]
        if flips:
            x = x.flip(flips)
        return x.permute(perm).contiguous()
    return run, theta is not None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu", action="store_true", help="also time the float64 CPU restatement once per case")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_preprocess: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    import preprocess_ref as R
    dev = torch.device("cuda:0")

    def lps(sp):
        A = np.diag([-sp[0], -sp[1], sp[2], 1.0])
        A[:3, 3] = (120.0, 95.0, -310.0)
        return A
    cases = {
        "ct": dict(C=1, shape=(512, 512, 90), dtype=torch.int16, affine=lps((0.79, 0.79, 5.0)), converter=None),
        "mr": dict(C=4, shape=(240, 240, 155), dtype=torch.float32, affine=lps((1.0, 1.0, 1.0)), converter="brats"),
    }
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    for name, c in cases.items():
        g = torch.Generator(device=dev).manual_seed(0)
        img = (torch.randn(c["C"], *c["shape"], generator=g, device=dev) * 300).to(c["dtype"])
        lbl = torch.randint(0, 4, (1, *c["shape"]), generator=g, device=dev, dtype=torch.uint8)
        A, pix = c["affine"], (1.0, 1.0, 1.0)
        oi, ol, _ = pkg.resample_orient(img, lbl, A, pix, "RAS", c["converter"])
        res = {"source": [c["C"], *c["shape"]], "output": list(oi.shape), "label_channels": ol.shape[0]}
        moved = img.numel() * img.element_size() + lbl.numel() + oi.numel() * 4 + ol.numel()
        # the kernel alone (outputs allocated, matrix planned) and the whole Python call (host plan + allocation + kernel)
        out_shape, mat, _ = pkg.preprocess.plan(c["shape"], A, pix, "RAS")
        m = (ctypes.c_double * 12)(*mat.reshape(-1).tolist())
        st = torch.cuda.current_stream().cuda_stream

        def kernel(with_label=True):
            pkg._capi.call("unetr_resample_orient", img.data_ptr(), int(img.dtype == torch.int16), lbl.data_ptr() if with_label else None,
                           c["C"], ol.shape[0] if with_label else 0, int(c["converter"] == "brats"), *c["shape"], m, *out_shape,
                           oi.data_ptr(), ol.data_ptr() if with_label else None, st)
        res["us"] = round(time_calls(kernel, args.iters), 1)
        res["bytes_moved"] = moved
        res["GBps"] = round(moved / (res["us"] * 1e-6) / 1e9, 1)
        res["image_only_us"] = round(time_calls(lambda: kernel(False), args.iters), 1)
        res["call_us"] = round(time_calls(lambda: pkg.resample_orient(img, lbl, A, pix, "RAS", c["converter"]), args.iters), 1)
        del oi, ol
        run, sampled = torch_route(R, img, A, pix)
        res["torch_route"] = "affine_grid + grid_sample + flip + permute" if sampled else "flip + permute (identity spacing)"
        res["torch_image_only_us"] = round(time_calls(run, args.iters), 1)
        if args.cpu:
            t0 = time.perf_counter()
            R.library_route(img.cpu(), A, pix, "RAS", "bilinear")
            R.library_route(lbl.cpu(), A, pix, "RAS", "nearest")
            res["cpu_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out[name] = res
        del img, lbl, run
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
