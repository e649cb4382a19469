"""Gradient clipping by global L2 norm on the device (csrc/grad_clip.hip), torch.nn.utils.clip_grad_norm_ semantics.

Two users.  ``optim.AdamW(max_grad_norm=...)`` measures the norm of the gradients it is about to apply -- the arena, or the
all-reduced communication buffer of the data-parallel step -- and hands the coefficient to the AdamW kernels in device memory:
two launches per step, the gradients are never rewritten, and the whole thing is part of a captured step.  ``clip_grad_norm_`` is
the free function for a loop of one's own around ``opt.step()``: it scales ``p.grad`` in place.

Everything is stream-ordered and device-resident.  The result is the clip row ``{norm, coef, max_norm, nonfinite}``: the norm from a
float64 sum of squares (within 1 ulp of the correctly rounded fp32 norm), ``coef = min(1, max_norm / (norm + 1e-6))`` in fp32 as torch
computes it.  The sum uses no atomics: the same gradients give the same bits."""
import math

import torch

from . import grad_arena
from ._capi import call

BLOCK = 8192                 # elements per workgroup of the sum-of-squares launch = per slot of its workspace (grad_clip.hip: GC_BLOCK)


def blocks_of(n):
    return (n + BLOCK - 1) // BLOCK


def check_max_norm(max_norm):
    """max_norm as a float: positive, +inf allowed (= measure, never scale); anything else is a ValueError"""
    v = float(max_norm)
    if math.isnan(v) or v <= 0.0:
        raise ValueError(f"max_norm must be a positive number (float('inf') measures without scaling), got {max_norm!r}")
    return v


def _stream():
    return torch.cuda.current_stream().cuda_stream


def new_row(device, max_norm):
    """a fresh clip row {0, 1, max_norm, 0} on `device`: a fill and one single-thread launch, no host-to-device copy"""
    row = torch.zeros(4, dtype=torch.float32, device=device)
    row[1] = 1.0
    call("unetr_grad_clip_set", row.data_ptr(), max_norm, _stream())
    return row


def range_table(offsets, params, pattern, device):
    """(table, rows, blocks) of the per-parameter ranges [offset, offset + numel) of the parameters in `pattern`: only those are read
    -- the arena slices of the others hold stale values"""
    rows, blocks = [], 0
    for p, o, has in zip(params, offsets, pattern):
        if has and p.numel():
            rows.append((o, o + p.numel(), blocks))
            blocks += blocks_of(p.numel())
    table = torch.tensor(rows, dtype=torch.int64, device=device) if rows else None
    return table, len(rows), blocks


def sumsq_ranges(src, table, nr, blocks, partials):
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("gradient source must be fp32 or bf16")
    call("unetr_grad_sumsq_ranges", src.data_ptr(), int(src.dtype == torch.bfloat16), table.data_ptr(), nr, blocks, partials.data_ptr(),
         partials.numel() * 8, _stream())


def sumsq_tensors(grads, partials):
    """one launch per (contiguous, non-empty) gradient tensor, each into its own workspace slots; returns the slots used"""
    used = 0
    for g in grads:
        if g.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("HIP gradient clipping needs fp32 or bf16 gradients")
        call("unetr_grad_sumsq", g.data_ptr(), int(g.dtype == torch.bfloat16), g.numel(), partials.data_ptr() + 8 * used,
             (partials.numel() - used) * 8, _stream())
        used += blocks_of(g.numel())
    return used


def finalize(partials, n, gscale, row):
    call("unetr_grad_clip_finalize", partials.data_ptr(), n, gscale, row.data_ptr(), _stream())


def _arena_of(params):
    """the flat arenas all of `params` write their gradients into, when every .grad IS its arena slice; else None"""
    flat = None
    for p in params:
        st = grad_arena.owner(p)
        f = st.flat if st is not None else None
        if f is None or (flat is not None and f is not flat):
            return None
        flat = f
    index = flat.get("_clip_index")
    if index is None:
        index = flat["_clip_index"] = {id(q): (i, o) for i, (q, o) in enumerate(zip(flat["params"], flat["offsets"]))}
    gbase = flat["grad"].data_ptr()
    for p in params:
        ent = index.get(id(p))
        if ent is None or p.grad.data_ptr() != gbase + 4 * ent[1] or p.grad.dtype != torch.float32:
            return None
    return flat, index


@torch.no_grad()
def clip_grad_norm_row_(parameters, max_norm, error_if_nonfinite=False):
    """``clip_grad_norm_`` returning the whole clip row, a device tensor ``{norm, coef, max_norm, nonfinite}``: the gradients have
    been multiplied by ``row[1]``."""
    max_norm = check_max_norm(max_norm)

    def check(row):
        if error_if_nonfinite and not math.isfinite(float(row[0])):          # (a host read: synchronises)
            raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be clipped")

    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        raise ValueError("clip_grad_norm_: no parameter has a gradient (and therefore no device to put the norm on)")
    dev = params[0].device
    if any(not p.grad.is_cuda or p.grad.device != dev for p in params):
        raise RuntimeError("HIP gradient clipping needs every gradient on one ROCm device (no CPU fallback)")
    if any(p.grad.dtype != torch.float32 for p in params):
        raise RuntimeError("clip_grad_norm_ scales fp32 gradients in place")
    row = new_row(dev, max_norm)
    arena = _arena_of(params)
    if arena is not None:
        flat, index = arena
        have = {index[id(p)][0] for p in params}
        pattern = tuple(i in have for i in range(len(flat["params"])))
        # the range tables live with the arena they describe (like the index above): another model, whatever its address, has its own
        tables = flat.setdefault("_clip_tables", {})
        ent = tables.get(pattern)
        if ent is None:
            ent = tables[pattern] = range_table(flat["offsets"], flat["params"], pattern, dev)
        table, nr, blocks = ent
        if nr:
            partials = torch.empty(blocks, dtype=torch.float64, device=dev)
            sumsq_ranges(flat["grad"], table, nr, blocks, partials)
            finalize(partials, blocks, 1.0, row)
            check(row)
            call("unetr_grad_scale_ranges", flat["grad"].data_ptr(), table.data_ptr(), nr, blocks, row.data_ptr() + 4, _stream())
        return row
    # per tensor.  A non-contiguous gradient is measured and scaled through a contiguous copy, written back afterwards
    work = [(p.grad, p.grad if p.grad.is_contiguous() else p.grad.contiguous()) for p in params if p.grad.numel()]
    if not work:
        return row
    partials = torch.empty(sum(blocks_of(c.numel()) for _, c in work), dtype=torch.float64, device=dev)
    used = sumsq_tensors([c for _, c in work], partials)
    finalize(partials, used, 1.0, row)
    check(row)
    for g, c in work:
        call("unetr_grad_scale", c.data_ptr(), c.numel(), row.data_ptr() + 4, _stream())
        if c is not g:
            g.copy_(c)
    return row


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ for device parameters on the HIP kernels: the gradients of ``parameters`` are scaled in place
    by ``min(1, max_norm / (total_norm + 1e-6))`` and the total L2 norm is returned as a 0-d device tensor.  One table-driven
    launch each for the norm and the scaling when every gradient is a slice of a model's gradient arena
    (``UNETR.use_flat_buffers``), else one launch per tensor; no host synchronisation either way.  Only ``norm_type=2`` exists.
    ``error_if_nonfinite=True`` reads the norm back -- it SYNCHRONISES with the device -- and raises RuntimeError when it is inf or
    NaN, before anything is scaled, as torch does."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only the L2 norm (norm_type=2) is implemented, got norm_type={norm_type!r}")
    return clip_grad_norm_row_(parameters, max_norm, error_if_nonfinite)[0]
