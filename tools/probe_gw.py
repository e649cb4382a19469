"""The grouped ViT weight-gradient launch alone (48 Linear problems of the 12 blocks at M token rows, operands warm in the MALL):
the plain gradient store, the fused AdamW epilogue, and the fused epilogue that also writes the transposed bf16 weight twins."""
import ctypes
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
capi = pkg._capi
from tools.probe_gemm_big import timeit  # noqa: E402

dev = torch.device("cuda:0")
M, H, MLP = int(os.environ.get("PROBE_M", 432)), 768, 3072
shapes = [(3 * H, H), (H, H), (MLP, H), (H, MLP)] * 12
arr = (capi.GroupedProblem * len(shapes))()
keep = []
flops = 0
for i, (N, K) in enumerate(shapes):
    dy = torch.randn(M, N, device=dev).bfloat16()
    x = torch.randn(M, K, device=dev).bfloat16()
    out = torch.empty(N, K, device=dev)
    keep += [dy, x, out]
    arr[i].dy, arr[i].x, arr[i].dw, arr[i].M, arr[i].N, arr[i].K = dy.data_ptr(), x.data_ptr(), out.data_ptr(), M, N, K
    flops += 2 * M * N * K
us = timeit(lambda: capi.call("unetr_gemm_bf16_grouped_wgrad", arr, len(shapes), torch.cuda.current_stream().cuda_stream), reps=3)
print(f"plain gradient store (32-token stages x 2, row-coalesced epilogue): {us:8.1f} us  {flops / us / 1e6:7.1f} TFLOP/s  "
      f"({sum(n * k for n, k in shapes) * 4 / us / 1e3:6.1f} GB/s of dW stores)", flush=True)

# the fused AdamW epilogue on one arena holding the 48 weights, without / with the transposed bf16 shadow (shadow_t)
offs, total = [], 0
for N, K in shapes:
    offs.append(total)
    total += N * K
p, g, m, v = (torch.zeros(total, device=dev) for _ in range(4))
p.normal_(0, 0.02)
shadow, shadow_t = p.bfloat16(), torch.zeros(total, device=dev, dtype=torch.bfloat16)
steps = torch.ones(len(shapes), device=dev)
arena = capi.AdamWArena(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(), steps.data_ptr(), total, 1e-4, 0.9, 0.999, 1e-8, 1e-5)
for i in range(len(shapes)):
    arr[i].dw = g.data_ptr() + 4 * offs[i]
sidx = (ctypes.c_int * len(shapes))(*range(len(shapes)))
for name, st in (("fused AdamW epilogue", None), ("fused AdamW epilogue + transposed twin", shadow_t.data_ptr())):
    us = timeit(lambda: capi.call("unetr_gemm_bf16_grouped_wgrad_adamw_t", arr, len(shapes), ctypes.byref(arena), sidx, st,
                                  torch.cuda.current_stream().cuda_stream), reps=3)
    nbytes = total * (26 + (2 if st else 0))          # p, m, v read and written (24 B), bf16 shadow (2 B), twin (2 B)
    print(f"{name}: {us:8.1f} us  {nbytes / us / 1e3:6.1f} GB/s of optimizer traffic", flush=True)
