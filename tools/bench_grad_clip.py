"""What gradient clipping by global norm costs on the MI355X (csrc/grad_clip.hip, optim.AdamW(max_grad_norm=...)), at the benchmark
configuration (bench.py: UNETR 96^3, hidden 768, 4 classes, bf16, batch 2).

    python tools/bench_grad_clip.py [--iters 200] [--steps 40] [--rounds 5] [--out profiles/grad_clip.txt]

One process, the candidates alternated --rounds times; every entry is listed per round, with its median and the repeat-to-repeat
spread (max - min) / median.
  norm passes, us per call of --iters back-to-back calls between two HIP events, and the bytes/s of the gradient bytes they read:
    * hip_norm_fp32 / hip_norm_bf16: the table-driven sum-of-squares launch + the finalize launch over the fp32 gradient arena / a
      bf16 buffer laid out like it (the data-parallel communication buffer), only the parameters that have a gradient;
    * torch_vector_norm_fp32 / _bf16: torch.linalg.vector_norm over the WHOLE flat buffer (one fused reduction of the same memory);
    * torch_clip_grad_norm_foreach: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm, foreach=True) on the arena views.
  steps, ms per step of --steps replays between two events: the captured unfused step unclipped and clipped (max_grad_norm = 12),
  and the captured fused unclipped step for context (clipping gives the fused epilogue up).
The norm passes above re-read ONE buffer back to back: the 185 MB bf16 buffer fits the 256 MiB Infinity Cache entirely, the 370 MB fp32
arena partly, so their bytes/s are cache-assisted rates, not the HBM rate -- the same for the torch reductions they are compared
with.  The "_cold" entries are the same four passes cycling over 6 (fp32) / 12 (bf16) copies of the buffer, 2.2 GB in all, so that
a copy has left the cache when its turn comes again: bytes/s from HBM.  What the pass costs inside a step, right after backward or
the all-reduce wrote the buffer, is the clipped-minus-unclipped step time.
The bound of the feature: the norm launches take no longer than torch's single-tensor vector_norm over the same bytes plus the larger
of 10 % and the measured spread.  The file says whether it held."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_seg_loss import time_launches  # noqa: E402

CFG = dict(in_channels=1, out_channels=4, img_size=(96, 96, 96), feature_size=16, hidden_size=768, mlp_dim=3072,
           num_heads=12, pos_embed="perceptron", norm_name="instance", res_block=True)


def build(pkg, dev, x, y, max_grad_norm, fuse):
    torch.manual_seed(1234)
    model = pkg.UNETRLogits(**CFG).to(dev)
    model.precision = "bf16"
    flat = model.use_flat_buffers()
    opt = pkg.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-5, flat=flat, max_grad_norm=max_grad_norm)
    step = pkg.TrainStep(model, pkg.DiceCELoss(to_onehot_y=True, softmax=True), opt, x, y, use_graph=True, fuse_update=fuse)
    return model, flat, opt, step


def time_steps(step, n):
    for _ in range(3):
        step.run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step.run()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) / n, 4)


def summary(vals):
    med = statistics.median(vals)
    return {"rounds": vals, "median": round(med, 4), "spread": round((max(vals) - min(vals)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip: no GPU")
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    from oracle.unetr_oracle import synthetic_volume
    dev = torch.device("cuda:0")
    x, y = synthetic_volume(2, 1, 96, 4, seed=0)
    x, y = x.to(dev), y.to(dev)

    plain = build(pkg, dev, x, y, None, False)
    clipped = build(pkg, dev, x, y, 12.0, False)
    fused = build(pkg, dev, x, y, None, True)
    model, flat, opt, step = clipped
    for _ in range(2):
        step.run()
    torch.cuda.synchronize()
    (pattern,) = list(opt._clip_tables)                      # the gradient pattern of the step: everything but the unused cls_token
    grad = flat["grad"]
    grad_bf16 = grad.bfloat16()
    counted = sum(p.numel() for p, has in zip(flat["params"], pattern) if has)
    mine = pkg.AdamW(model.parameters(), flat=flat, max_grad_norm=12.0)          # its own clip row: the step's is not disturbed
    views = [(p, grad[o:o + p.numel()].view_as(p)) for p, o, has in zip(flat["params"], flat["offsets"], pattern) if has]

    def torch_clip():
        torch.nn.utils.clip_grad_norm_([p for p, _ in views], 1e30, foreach=True)

    norm_routes = {
        "hip_norm_fp32": (lambda: mine._clip_arena(pattern, grad, 1.0), counted * 4),
        "torch_vector_norm_fp32": (lambda: torch.linalg.vector_norm(grad), grad.numel() * 4),
        "hip_norm_bf16": (lambda: mine._clip_arena(pattern, grad_bf16, 1.0), counted * 2),
        "torch_vector_norm_bf16": (lambda: torch.linalg.vector_norm(grad_bf16), grad.numel() * 2),
        "torch_clip_grad_norm_foreach": (torch_clip, counted * 4),
    }
    # cold: every call reads another copy; a copy is read again after 2.2 GB of other copies went through the 256 MiB cache
    copies = {"fp32": [grad.clone() for _ in range(6)], "bf16": [grad_bf16.clone() for _ in range(12)]}
    turn = {"n": 0}

    def cycling(kind, fn):
        def call():
            turn["n"] += 1
            fn(copies[kind][turn["n"] % len(copies[kind])])
        return call

    for kind, esz in (("fp32", 4), ("bf16", 2)):
        norm_routes[f"hip_norm_{kind}_cold"] = (cycling(kind, lambda b: mine._clip_arena(pattern, b, 1.0)), counted * esz)
        norm_routes[f"torch_vector_norm_{kind}_cold"] = (cycling(kind, torch.linalg.vector_norm), grad.numel() * esz)
    step_routes = {"captured_unfused_unclipped_ms": plain[3], "captured_unfused_clipped_ms": clipped[3], "captured_fused_unclipped_ms": fused[3]}
    res = {k: [] for k in list(norm_routes) + list(step_routes)}
    for _ in range(args.rounds):
        for p, v in views:
            p.grad = v
        for name, (fn, _) in norm_routes.items():
            res[name].append(time_launches(fn, args.iters))
        for p, _ in views:
            p.grad = None
        for name, st in step_routes.items():
            res[name].append(time_steps(st, args.steps))
    mine._clip_arena(pattern, grad, 1.0)                      # (the arena as the last replay left it: what the float64 check below reads)
    torch.cuda.synchronize()
    hip_norm = float(mine.grad_norm())
    ref_norm = float(torch.linalg.vector_norm(torch.cat([v.reshape(-1) for _, v in views]).double()))

    out = {"device": torch.cuda.get_device_name(0), "config": "bench.py c2: UNETR 96^3 hidden 768, bf16, batch 2", "iters": args.iters,
           "steps": args.steps, "arena_floats": grad.numel(), "floats_with_gradient": counted,
           "launches": {"clipped": clipped[3].launch, "unclipped": plain[3].launch, "fused": fused[3].launch},
           "norm_check": {"hip": hip_norm, "float64": ref_norm}}
    for name, vals in res.items():
        s = summary(vals)
        if name in norm_routes:
            s["unit"] = "us per call"
            s["bytes"] = norm_routes[name][1]
            s["GB_per_s"] = round(norm_routes[name][1] / (s["median"] * 1e-6) / 1e9, 1)
        else:
            s["unit"] = "ms per step"
        out[name] = s
    lines = [json.dumps(out, indent=1), ""]
    for kind in ("fp32", "bf16", "fp32_cold", "bf16_cold"):
        hip, ref = out[f"hip_norm_{kind}"], out[f"torch_vector_norm_{kind}"]
        slack = max(0.10, hip["spread"], ref["spread"])
        ok = hip["median"] <= ref["median"] * (1.0 + slack)
        lines.append(f"bound ({kind}): norm + finalize launches {hip['median']} us ({hip['GB_per_s']} GB/s) against torch.linalg.vector_norm "
                     f"{ref['median']} us ({ref['GB_per_s']} GB/s), slack {slack:.2%}: {'HELD' if ok else 'MISSED'}")
    lines.append("(fp32 / bf16: one buffer re-read back to back while it is resident in the 256 MiB Infinity Cache -- all of the bf16 buffer, part "
                 "of the fp32 arena: cache-assisted bytes/s on both sides of the comparison; _cold: cycling over 2.2 GB of copies, bytes/s from HBM)")
    d = out["captured_unfused_clipped_ms"]["median"] - out["captured_unfused_unclipped_ms"]["median"]
    lines.append(f"clipping costs the captured unfused step {d * 1e3:.1f} us ({out['captured_unfused_unclipped_ms']['median']} -> "
                 f"{out['captured_unfused_clipped_ms']['median']} ms); the fused unclipped step it gives up runs at "
                 f"{out['captured_fused_unclipped_ms']['median']} ms")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
