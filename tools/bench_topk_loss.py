"""GPU time of the top-k cross entropy and of the radix select under it (csrc/topk_loss.hip, csrc/select.hip) at the training
shapes, and of percentile() on a CT-sized volume.

    python tools/bench_topk_loss.py [--iters 200] [--rounds 3] [--no-percentile]
    python tools/bench_topk_loss.py --single          # one call of each route, for a kernel trace (rocprofv3 --kernel-trace --stats)

Prints ONE JSON line.  Shapes: B=2, 96^3, C=4 and C=14, seeded logits and labels, k = 10.  Per shape, forward + backward through
autograd (criterion(logits, y).backward()), every route in the same process, alternated --rounds times, each entry the median of
--iters warmed calls by HIP events (eager routes: --iters / 5 calls):
  * "topk_us", "dice_topk_us": TopKLoss and DiceTopKLoss;
  * "segloss_dicece_us": SegLoss with its DiceCE defaults -- the parent's unchanged kernels, so that what the selection costs on top
    of a streaming loss is visible;
  * "eager_topk_us": cross_entropy(reduction="none") -> torch.topk -> mean in eager torch;  "eager_dice_topk_us": that plus an
    eager Dice;
  * "select": unetr_select_kth alone on the loss map of that shape (B*V values, K-th largest), 200 back-to-back calls between two
    events, with the LDS-contention remedy of the histogram passes ("copies8_merge_us") and without it ("plain_us":
    UNETR_SELECT_PLAIN_HIST), alternated; the same on uniform random bits, where the first digit spreads over all 256 bins.
"percentile": percentile(x, (0.5, 99.5)) on a 512 x 512 x 300 float32 volume against torch.sort of the same tensor (+ the same
interpolation) and against np.percentile with the copy to the host included."""
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_seg_loss import eager_dice, step_of, time_calls, time_launches  # noqa: E402


def eager_topk(logits, label, k=10.0):
    ce = F.cross_entropy(logits, label[:, 0].long(), reduction="none").reshape(-1)
    return torch.topk(ce, max(1, int(ce.numel() * k / 100.0)), sorted=False).values.mean()


def eager_dice_topk(logits, label, k=10.0):
    t = F.one_hot(label[:, 0].long(), logits.shape[1]).movedim(-1, 1).float()
    return eager_dice(torch.softmax(logits, 1), t) + eager_topk(logits, label, k)


def loss_map(pkg, logits, label):
    """the per-voxel values of a TopKLoss forward, as the select sees them"""
    Fn, capi = pkg.functional, pkg._capi
    B, C = logits.shape[:2]
    V = logits[0, 0].numel()
    d = capi.TopKCEDesc(B=B, C=C, V=V)
    values = torch.empty(B * V, device=logits.device)
    out, coef, k = torch.empty(4, device=logits.device), torch.empty(4, device=logits.device), torch.full((1,), 10.0, device=logits.device)
    ws = Fn.workspace(logits.device)
    capi.call("unetr_topkce_fwd", ctypes.byref(d), logits.data_ptr(), label.data_ptr(), k.data_ptr(), values.data_ptr(), out.data_ptr(),
              coef.data_ptr(), ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    return values


def select_call(pkg, x, rank, flags):
    Fn, capi = pkg.functional, pkg._capi
    ws, res = Fn.workspace(x.device), torch.empty(3, dtype=torch.int32, device=x.device)
    st = torch.cuda.current_stream().cuda_stream
    return lambda: capi.call("unetr_select_kth", x.data_ptr(), x.numel(), None, rank, flags, res.data_ptr(), ws.data_ptr(), ws.numel() * 4, st)


def bench_select(pkg, x, rank, iters, rounds):
    capi = pkg._capi
    on, off = select_call(pkg, x, rank, capi.SELECT_LARGEST), select_call(pkg, x, rank, capi.SELECT_LARGEST | capi.SELECT_PLAIN_HIST)
    r = {"n": x.numel(), "copies8_merge_us": [], "plain_us": []}
    for _ in range(rounds):
        r["copies8_merge_us"].append(time_launches(on, iters))
        r["plain_us"].append(time_launches(off, iters))
    return r


def sort_percentile(x, q):
    v = torch.sort(x.reshape(-1)).values
    n = v.numel()
    out = []
    for p in q:
        pos = p / 100.0 * (n - 1)
        lo = int(pos)
        out.append(v[lo].double() + (v[min(lo + 1, n - 1)].double() - v[lo].double()) * (pos - lo))
    return torch.stack(out)


def bench_percentile(pkg, dev, iters):
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(300, 512, 512, generator=gen, device=dev) * 400 - 200
    q = (0.5, 99.5)
    r = {"shape": list(x.shape), "q": list(q)}
    r["hip_percentile_us"] = time_calls(lambda: pkg.percentile(x, q), iters)
    try:
        r["torch_sort_us"] = time_calls(lambda: sort_percentile(x, q), 10)
    except RuntimeError as e:                                  # a comparison that cannot run is reported, not hidden
        r["torch_sort_error"] = str(e).splitlines()[0][:200]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = np.percentile(x.cpu().numpy(), q)
        ts.append((time.perf_counter() - t0) * 1e6)
    r["numpy_with_copy_us"] = round(statistics.median(ts), 1)
    got = pkg.percentile(x, q).cpu().numpy()
    r["hip_vs_numpy_float32_interp_relerr"] = float(np.max(np.abs(got - want) / np.abs(want)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-percentile", action="store_true")
    ap.add_argument("--single", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_loss: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    dev = torch.device("cuda:0")
    OH = dict(to_onehot_y=True, softmax=True)
    out = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    B, S = 2, 96
    for C in (14,) if args.single else (4, 14):
        gen = torch.Generator(device=dev).manual_seed(C)
        logits = (torch.randn(B, C, S, S, S, generator=gen, device=dev) * 2).requires_grad_(True)
        label = torch.randint(0, C, (B, 1, S, S, S), generator=gen, device=dev).float()
        values = loss_map(pkg, logits.detach(), label)
        rank = values.numel() // 10 - 1
        if args.single:
            capi = pkg._capi
            for _ in range(2):                                  # the second pass of each is the warmed one
                step_of(pkg.TopKLoss(k=10.0, **OH), logits, label)()
                select_call(pkg, values, rank, capi.SELECT_LARGEST)()
                select_call(pkg, values, rank, capi.SELECT_LARGEST | capi.SELECT_PLAIN_HIST)()
            torch.cuda.synchronize()
            out["single"] = "one TopKLoss forward + backward and one select of each kind, twice"
            break
        routes = {"topk_us": step_of(pkg.TopKLoss(k=10.0, **OH), logits, label),
                  "dice_topk_us": step_of(pkg.DiceTopKLoss(k=10.0, **OH), logits, label),
                  "segloss_dicece_us": step_of(pkg.SegLoss(**OH), logits, label)}
        eager = {"eager_topk_us": eager_topk, "eager_dice_topk_us": eager_dice_topk}
        res = {name: [] for name in list(routes) + list(eager)}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                res[name].append(time_calls(fn, args.iters))
            for name, fn in eager.items():
                def eager_step():
                    logits.grad = None
                    fn(logits, label).backward()
                try:
                    res[name].append(time_calls(eager_step, max(args.iters // 5, 5)))
                except RuntimeError as e:                      # an eager comparison that cannot run is reported, not hidden
                    res[name].append(str(e).splitlines()[0][:200])
        res["select"] = {"loss_map": bench_select(pkg, values, rank, args.iters, args.rounds)}
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (values.numel(),), generator=gen, device=dev, dtype=torch.int64).to(torch.int32)
        res["select"]["uniform_bits"] = bench_select(pkg, bits.view(torch.float32), rank, args.iters, args.rounds)
        out[f"B{B}_C{C}_{S}^3"] = res
        del logits, label, values, bits
        torch.cuda.empty_cache()
    if not args.no_percentile and not args.single:
        out["percentile"] = bench_percentile(pkg, dev, max(args.iters // 10, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
