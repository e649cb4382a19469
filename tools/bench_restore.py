"""GPU time of one preprocess.restore_native call (prediction on the 1 mm RAS grid -> the scan's own voxel grid).

    python tools/bench_restore.py [--iters 20]

Prints ONE JSON line: per case the median of --iters warmed kernel launches timed with HIP events (us; call_us is the whole
Python call with the host inverse and the allocation), the bytes the kernel must move (source once + output once) and the
implied rate, and the same result computed with torch on the same GPU (fp32): torch.nn.functional.affine_grid + grid_sample
(bilinear, border) of the C score channels onto the native grid, then argmax / threshold + the BraTS rule.  Cases, the
geometries of tools/bench_preprocess.py backwards:
  ct2, ct14: 2 / 14 x 405x405x446 float32 scores at 1 mm RAS -> 512x512x90 at (0.79, 0.79, 5.0) mm LPS, linear + argmax
  mr:        4 x 240x240x155 float32 logits, 1 mm RAS -> LPS (a pure reorientation: the one-tap path), sigmoid + brats
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_preprocess import time_calls  # noqa: E402


def torch_route(R, scores, geom, post, brats):
    """the yardstick: a closure that maps `scores` [C, d, h, w] onto the native grid with torch ops only (fp32)"""
    Minv = np.vstack([geom.inverse_matrix(), [0.0, 0.0, 0.0, 1.0]])
    th = R.to_norm_affine_matrix(geom.full_shape) @ Minv @ np.linalg.inv(R.to_norm_affine_matrix(geom.native_shape))
    rev = [2, 1, 0, 3]
    theta = torch.as_tensor(th[rev][:, rev][:3], dtype=torch.float32, device=scores.device)[None]
    size = [1, scores.shape[0], *geom.native_shape]

    def run():
        grid = F.affine_grid(theta, size, align_corners=False)
        v = F.grid_sample(scores[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0]
        if post == "argmax":
            return v.argmax(0, keepdim=True).to(torch.uint8)
        ch = v >= 0
        if not brats:
            return ch.to(torch.uint8)
        out = torch.zeros(1, *geom.native_shape, dtype=torch.uint8, device=scores.device)
        out[0][ch[2]] = 1
        out[0][ch[1]] = 2
        out[0][ch[3]] = 3
        return out
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    import preprocess_ref as R
    dev = torch.device("cuda:0")

    def lps(sp):
        A = np.diag([-sp[0], -sp[1], sp[2], 1.0])
        A[:3, 3] = (120.0, 95.0, -310.0)
        return A
    ct, mr = dict(shape=(512, 512, 90), affine=lps((0.79, 0.79, 5.0))), dict(shape=(240, 240, 155), affine=lps((1.0, 1.0, 1.0)))
    cases = {
        "ct2": dict(ct, C=2, post="argmax", converter=None),
        "ct14": dict(ct, C=14, post="argmax", converter=None),
        "mr": dict(mr, C=4, post="sigmoid", converter="brats"),
    }
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    for name, c in cases.items():
        geom = pkg.preprocess.geometry(c["shape"], c["affine"], (1.0, 1.0, 1.0), "RAS")
        g = torch.Generator(device=dev).manual_seed(0)
        scores = torch.randn(c["C"], *geom.full_shape, generator=g, device=dev)
        kw = dict(mode="linear", post=c["post"], label_converter=c["converter"])
        res_t = pkg.restore_native(scores, geom, **kw)
        res = {"source": list(scores.shape), "output": list(res_t.shape), "post": c["post"], "label_converter": c["converter"]}
        moved = scores.numel() * 4 + res_t.numel()
        # the kernel alone (output allocated, matrix inverted) and the whole Python call (host inverse + allocation + kernel)
        rg = pkg._capi.RestoreGeom()
        rg.m[:] = geom.inverse_matrix().reshape(-1).tolist()
        rg.full[:], rg.origin[:], rg.crop[:] = geom.full_shape, geom.crop_origin, geom.crop_shape
        st = torch.cuda.current_stream().cuda_stream

        def kernel(post=pkg.preprocess.RESTORE_POST[c["post"]], brats=int(c["converter"] == "brats"), dst=res_t):
            pkg._capi.call("unetr_restore_native", scores.data_ptr(), 0, c["C"], rg, *c["shape"], 1, post, brats, dst.data_ptr(), st)
        res["us"] = round(time_calls(kernel, args.iters), 1)
        res["bytes_moved"] = moved
        res["GBps"] = round(moved / (res["us"] * 1e-6) / 1e9, 1)
        res["call_us"] = round(time_calls(lambda: pkg.restore_native(scores, geom, **kw), args.iters), 1)
        plain = torch.empty(c["C"], *c["shape"], device=dev)
        res["scores_only_us"] = round(time_calls(lambda: kernel(0, 0, plain), args.iters), 1)      # post=None: C float32 channels stored
        del plain
        run = torch_route(R, scores, geom, c["post"], c["converter"] == "brats")
        same = (run() == res_t).float().mean().item()
        res["torch_agreement"] = round(same, 6)
        res["torch_us"] = round(time_calls(run, args.iters), 1)
        out[name] = res
        del scores, res_t, run
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
