"""GPU time of one validation pass over one volume: the per-window sliding_window_inference against SlidingWindowInferer
(DESIGN.md section 14).

    python tools/bench_inference.py [--reps 5] [--overlaps 0.25 0.8] [--size 314 214 234]

Prints ONE JSON line.  Model: the full-size network (hidden 768, 96^3 window, 14 classes, precision "bf16", flat buffers),
sw_batch_size 4, one seeded volume (default 314x214x234), Gaussian blending.  Per overlap, four routes are timed with HIP events
around WHOLE calls after every shape has been warmed (graphs captured), alternated in one process, --reps repetitions each;
reported as median and [min, max] in ms:
  function        the per-window sliding_window_inference (one forward per 4 windows dispatched from Python, one
                  unetr_sw_accumulate launch per window)
  inferer_eager   SlidingWindowInferer(use_graph=False): batched gather / accumulate, eager forward
  inferer_graph   SlidingWindowInferer(use_graph=True), post=None
  onehot_torch    function + torch argmax + one_hot (AsDiscrete(argmax=True, to_onehot=True) as separate passes)
  onehot_fused    SlidingWindowInferer(use_graph=True), post="onehot"
and, for the two streaming kernels, the bytes each must move and the implied rate against the 8 TB/s of HBM:
  accumulate_batch   per row of 4 windows: seg + importance read once, the covered out / count voxels read and written once
                     (upper bound: overlap inside a row makes the true traffic smaller); time = (advance + accumulate) loop over
                     the real table minus an advance-only loop, per row
  finalize_post      out read and written once, count read once (post=None and "onehot" move the same bytes)
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CFG = dict(in_channels=1, out_channels=14, img_size=(96, 96, 96), feature_size=16, hidden_size=768, mlp_dim=3072,
           num_heads=12, pos_embed="perceptron", norm_name="instance", res_block=True)
ROI = (96, 96, 96)
HBM_BPS = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--overlaps", type=float, nargs="+", default=[0.25, 0.8])
    ap.add_argument("--size", type=int, nargs=3, default=[314, 214, 234])
    ap.add_argument("--sw-batch-size", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = pkg.UNETRLogits(**CFG).to(dev)
    model.precision = "bf16"
    model.use_flat_buffers()
    n, C = args.sw_batch_size, CFG["out_channels"]
    x = torch.randn(1, 1, *args.size, generator=torch.Generator().manual_seed(1)).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "volume": args.size, "window": list(ROI), "classes": C, "sw_batch_size": n,
           "precision": "bf16", "mode": "gaussian", "reps": args.reps, "overlaps": {}}
    s = torch.cuda.current_stream().cuda_stream
    for overlap in args.overlaps:
        eager = pkg.SlidingWindowInferer(ROI, n, overlap=overlap, mode="gaussian", use_graph=False)
        graph = pkg.SlidingWindowInferer(ROI, n, overlap=overlap, mode="gaussian", use_graph=True)
        function = lambda: pkg.sliding_window_inference(x, ROI, n, model, overlap=overlap, mode="gaussian")
        routes = {
            "function": function,
            "inferer_eager": lambda: eager(x, model),
            "inferer_graph": lambda: graph(x, model),
            "onehot_torch": lambda: F.one_hot(torch.argmax(function(), dim=1), C).movedim(-1, 1).float(),
            "onehot_fused": lambda: graph(x, model, post="onehot"),
        }
        for fn in routes.values():                      # warm every shape, capture every graph
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(routes["function"](), routes["inferer_graph"]()))
        times = {k: [] for k in routes}
        for _ in range(args.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn))
        table_cpu, counts = pkg.inference.plan_window_table(1, args.size, ROI, overlap, n)
        res = {"windows": sum(counts), "rows": len(counts), "graph_equals_function": same, "inferer_stats": dict(graph.stats)}
        res.update({k: summary(v) for k, v in times.items()})
        med = {k: statistics.median(v) for k, v in times.items()}
        res["speedup_graph_vs_function"] = round(med["function"] / med["inferer_graph"], 2)
        res["speedup_onehot_fused_vs_torch"] = round(med["onehot_torch"] / med["onehot_fused"], 2)
        # ---- the two streaming kernels alone
        D, H, W = args.size
        V = D * H * W
        rv = ROI[0] * ROI[1] * ROI[2]
        table = table_cpu.to(dev)
        sums = torch.zeros(1, C, D, H, W, device=dev)
        cnt = torch.zeros(1, D, H, W, device=dev)
        seg = torch.randn(n, C, *ROI, device=dev)
        imp = pkg.inference._device_importance_map(ROI, "gaussian", 0.125, dev)
        vol = pkg._capi.SwVolume()
        vol.out, vol.count, vol.table = sums.data_ptr(), cnt.data_ptr(), table.data_ptr()
        vol.B, vol.Cin, vol.C, vol.Di, vol.Hi, vol.Wi, vol.D, vol.H, vol.W = 1, 1, C, D, H, W, D, H, W
        vol.rows, vol.cursor = len(counts), -1
        host = torch.frombuffer(bytearray(bytes(vol)), dtype=torch.uint8)
        desc = host.to(dev)

        def loop(accumulate):
            desc.copy_(host)
            for _ in counts:
                pkg._capi.call("unetr_sw_advance", desc.data_ptr(), s)
                if accumulate:
                    pkg._capi.call("unetr_sw_accumulate_batch", desc.data_ptr(), seg.data_ptr(), imp.data_ptr(), n, C, *ROI, s)
        loop(True)
        t_acc = statistics.median([timed(lambda: loop(True)) for _ in range(args.reps)])
        t_adv = statistics.median([timed(lambda: loop(False)) for _ in range(args.reps)])
        per_row_us = (t_acc - t_adv) * 1e3 / len(counts)
        acc_bytes = n * rv * 4 * (C + 1 + 2 * C + 2)
        res["accumulate_batch"] = {"us_per_row": round(per_row_us, 1), "bytes_per_row_upper_bound": acc_bytes,
                                   "TBps": round(acc_bytes / (per_row_us * 1e-6) / 1e12, 2),
                                   "fraction_of_8TBps": round(acc_bytes / (per_row_us * 1e-6) / HBM_BPS, 3)}
        fin_bytes = V * 4 * (2 * C + 1)
        for name, post in (("finalize_post_logits", 0), ("finalize_post_onehot", 1)):
            ts = []
            for _ in range(args.reps + 1):
                cnt.fill_(1.0)
                ts.append(timed(lambda: pkg._capi.call("unetr_sw_finalize_post", sums.data_ptr(), cnt.data_ptr(), None, 1, C, V, post, s)))
            us = statistics.median(ts[1:]) * 1e3
            res[name] = {"us": round(us, 1), "bytes": fin_bytes, "TBps": round(fin_bytes / (us * 1e-6) / 1e12, 2),
                         "fraction_of_8TBps": round(fin_bytes / (us * 1e-6) / HBM_BPS, 3)}
        out["overlaps"][str(overlap)] = res
        del sums, cnt, seg, eager, graph, routes
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
