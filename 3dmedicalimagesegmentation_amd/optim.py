"""AdamW with torch.optim.AdamW semantics (unetr_segmentation_3d.py:522: lr from the CLI, weight_decay=1e-5,
betas (0.9, 0.999), eps 1e-8, amsgrad off) running on the HIP kernel ``unetr_adamw`` (csrc/norm_misc.hip).

Per-parameter step counters (a parameter whose grad is None does not step, as in torch) live in one device
tensor and are advanced by a single masked add, so ``step()`` never synchronises with the host and can be
captured in a hipGraph together with forward and backward.

``flat=model.use_flat_buffers()``: parameters, gradients and both moments live in flat arenas, and one kernel
launch covers every contiguous run of parameters that received a gradient (2 launches for the full model:
MONAI's unused ``cls_token`` splits the arena), instead of one launch per tensor.

The scalars that change during a run live on the device too: one ``hyper`` row ``{lr, weight_decay, t, reserved}`` per param group,
read by every AdamW kernel when it RUNS.  ``sync_hyper()`` uploads ``group["lr"]`` / ``group["weight_decay"]`` when they changed (a
``torch.optim.lr_scheduler`` keeps working under hipGraph replay), ``set_schedule()`` moves the schedule itself into the captured
step (it rides on the step-counter launch), and ``state_dict()`` / ``load_state_dict()`` speak torch.optim.AdamW's schema in both
modes, loading in place so that captured graphs stay valid.

``max_grad_norm=``: the gradients are clipped by their global L2 norm (torch.nn.utils.clip_grad_norm_ semantics, grad_clip.py) inside
``step()``: a sum-of-squares launch over exactly the gradients about to be applied and a one-workgroup finalize write the clip row
``{norm, coef, max_norm, nonfinite}`` in device memory, and every AdamW launch multiplies its gradients by ``coef`` as it reads them
(``unetr_adamw_hyper_clip``) -- the gradients themselves are not rewritten.  Two launches more per step, none when it is off."""
import ctypes
import math
import struct

import torch

from . import functional as Fn
from . import grad_clip
from ._capi import LrSchedule, call

SCHEDULES = {"constant": 0, "warmup_cosine": 1, "poly": 2}
# what torch.optim.AdamW expects to find in a param group it loads (its __setstate__ would otherwise default to the coupled L2 form)
_TORCH_GROUP_KEYS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                         decoupled_weight_decay=True)


def _f32(x):
    """x rounded to float32 (what a by-value float kernel argument or a device scalar holds), as a Python float"""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def schedule_lr(sched, s):
    """The learning rate of optimizer step ``s`` (0-based) under the schedule description ``sched`` (AdamW.set_schedule): the formula
    of the in-graph schedule (include/unetr_hip.h: unetr_lr_schedule) in Python floats, rounded once to float32."""
    kind, warm, total = SCHEDULES[sched["kind"]], float(sched["warmup"]), float(sched["total"])
    s = float(s)
    f = 1.0
    if kind == 1:
        if s < warm:
            f = s / max(1.0, warm)
        else:
            f = 0.5 * (1.0 + math.cos(math.pi * min(1.0, (s - warm) / max(1.0, total - warm))))
    elif kind == 2:
        f = (1.0 - min(s, total) / total) ** float(sched["power"])
    return max(_f32(sched["min_lr"]), _f32(_f32(sched["base_lr"]) * f))


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, flat=None, max_grad_norm=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        # None: no clipping, no extra launch; a positive number: clip the global gradient norm to it; float("inf"): measure only
        self.max_grad_norm = None if max_grad_norm is None else grad_clip.check_max_norm(max_grad_norm)
        self._clip = None        # device tensor [4]: the clip row {norm, coef, max_norm, nonfinite}, written by the finalize launch
        self._clip_uploaded = None   # max_norm as last written to the row by the host
        self._clip_ws = None     # per-tensor path: the float64 workspace of the sum-of-squares launches
        self._clip_ws_outgrown = []   # smaller workspaces it replaced, kept alive: a captured step may still write them
        self._clip_tables = {}   # arena paths: pattern -> (table, rows, blocks, workspace)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._steps = {}   # group index -> flat device tensor of per-parameter step counts
        self._masks = {}   # (group index, pattern) -> 0/1 increment tensor
        self._hyper = None       # device tensor [groups, 4]: {lr, weight_decay, t, reserved} per group, read by the kernels
        self._uploaded = [[None, None] for _ in self.param_groups]      # (lr, weight_decay) as float32, last written to the row by the host
        self._schedule = [None] * len(self.param_groups)               # per group: (description dict, LrSchedule) once set_schedule ran
        self._captured = False   # a hipGraph capture has recorded launches of this optimizer (their by-value arguments are frozen)
        self._runs_captured = set()  # flat mode: (first, last) parameter index of every run a captured launch steps with ONE shared counter
        self._flat = flat
        self._flat_state = None
        if flat is not None:
            if len(self.param_groups) != 1 or [id(p) for p in self.param_groups[0]["params"]] != [id(p) for p in flat["params"]]:
                raise ValueError("flat= needs a single param group holding model.parameters() in order")
            self._host_steps = [0] * len(flat["params"])

    # ---- device-resident hyper-parameters --------------------------------------------------------------------------------
    def _device(self):
        return self._flat["param"].device if self._flat is not None else self.param_groups[0]["params"][0].device

    def _hyper_ptr(self, gi):
        return self._hyper.data_ptr() + 16 * gi

    def _step_tensor(self, gi, dev):
        steps = self._steps.get(gi)
        if steps is None:
            steps = self._steps[gi] = torch.zeros(len(self.param_groups[gi]["params"]), dtype=torch.float32, device=dev)
        return steps

    def sync_hyper(self):
        """Write ``group["lr"]`` / ``group["weight_decay"]`` of every group to its device row if they differ from what was last
        uploaded: a stream-ordered single-thread launch with the values as arguments, no host synchronisation.  Called by every
        stepping entry point and by ``TrainStep.run()`` before a replay.  While the current stream is capturing nothing may be
        uploaded -- the write would become part of the graph and reset the rate on every replay -- so a pending change raises
        there.  With an in-graph schedule attached (``set_schedule``) ``group["lr"]`` is not read."""
        capturing = torch.cuda.is_current_stream_capturing()
        if len(self._uploaded) != len(self.param_groups):
            if self._hyper is not None:
                raise RuntimeError("AdamW: param groups cannot be added after the first step (one device row per group exists)")
            self._uploaded = [[None, None] for _ in self.param_groups]
            self._schedule = [None] * len(self.param_groups)
        if self._hyper is None:
            if capturing:
                raise RuntimeError("AdamW: the hyper-parameter row does not exist yet and cannot be created while a hipGraph is being "
                                   "captured; run one eager step (or sync_hyper()) before the capture")
            self._hyper = torch.zeros(len(self.param_groups), 4, dtype=torch.float32, device=self._device())
        for gi, group in enumerate(self.param_groups):
            have = self._uploaded[gi]
            lr = None if self._schedule[gi] is not None else _f32(group["lr"])
            wd = _f32(group["weight_decay"])
            fields = (1 if lr is not None and lr != have[0] else 0) | (2 if wd != have[1] else 0)
            if not fields:
                continue
            if capturing:
                raise RuntimeError("AdamW.sync_hyper: lr / weight_decay changed on the host while a hipGraph is being captured -- the "
                                   "upload would be replayed with every step; call sync_hyper() before the capture")
            if (lr is not None and lr < 0) or wd < 0:
                raise ValueError("invalid AdamW hyper-parameter")
            call("unetr_adamw_hyper_set", self._hyper_ptr(gi), fields, lr or 0.0, wd, 0.0, torch.cuda.current_stream().cuda_stream)
            self._uploaded[gi] = [lr if fields & 1 else have[0], wd]

    def set_schedule(self, kind, *, warmup=0, total=None, power=0.9, min_lr=0.0):
        """Attach the in-graph learning-rate schedule ``lr(s) = max(min_lr, base_lr * f(s))``, s = optimizer steps taken so far, to
        every group (``base_lr`` = the group's ``lr`` now).  kind: "constant" (f = 1), "warmup_cosine" (linear 0 -> 1 over ``warmup``
        steps, then half a cosine down to 0 at ``total``), "poly" (f = (1 - s / total) ** power).  The step-counter launch computes
        it on the device, so a captured step schedules itself with no extra launch and no host work; the description is a launch
        argument, hence it must be attached BEFORE a TrainStep captures."""
        if kind not in SCHEDULES:
            raise ValueError(f"unknown schedule {kind!r}: one of {sorted(SCHEDULES)}")
        if self._captured:
            raise RuntimeError("set_schedule: a captured step already uses this optimizer (the schedule is a launch argument frozen "
                               "in the graph); attach the schedule before TrainStep captures")
        if total is None:
            if kind != "constant":
                raise ValueError(f"schedule {kind!r} needs total=")
            total = 0
        if warmup < 0 or total < 0 or min_lr < 0 or (kind == "poly" and total <= 0):
            raise ValueError("invalid schedule")
        for gi, group in enumerate(self.param_groups):
            desc = dict(kind=kind, warmup=int(warmup), total=int(total), power=float(power), min_lr=float(min_lr), base_lr=float(group["lr"]))
            self._attach(gi, desc)

    def _attach(self, gi, desc):
        self._schedule[gi] = (desc, LrSchedule(SCHEDULES[desc["kind"]], desc["base_lr"], desc["min_lr"], desc["warmup"], desc["total"], desc["power"]))
        self._uploaded[gi][0] = None

    def schedule_lr(self, s, group=0):
        """the rate the attached schedule gives optimizer step ``s`` (0-based): the device formula on the host, for logging and tests"""
        if self._schedule[group] is None:
            return _f32(self.param_groups[group]["lr"])
        return schedule_lr(self._schedule[group][0], s)

    def current_lr(self, group=0):
        """the learning rate in device memory: what the last step used (synchronises with the device)"""
        if self._hyper is None:
            return self.schedule_lr(0, group)
        return float(self._hyper[group, 0])

    # ---- gradient clipping by global norm ----------------------------------------------------------------------------------
    def set_max_grad_norm(self, max_norm):
        """Change the clipping threshold: a stream-ordered single-thread write of the clip row's ``max_norm`` (no host
        synchronisation), which the finalize launch READS when it runs -- legal between replays of a captured step, which then
        clips to the new value.  ``float("inf")`` = measure, never scale.  While the current stream is capturing the write would
        become part of the graph, so it raises there (the rule of ``sync_hyper``).  Switching clipping on or off (``None``) changes
        which launches a step makes: only before a TrainStep captures."""
        on = max_norm is not None
        v = grad_clip.check_max_norm(max_norm) if on else None
        if on != (self.max_grad_norm is not None) and self._captured:
            raise RuntimeError("set_max_grad_norm: a captured step already uses this optimizer (whether it clips is frozen in the "
                               "graph); switch clipping on or off before TrainStep captures")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing() and v != self.max_grad_norm:
            raise RuntimeError("AdamW.set_max_grad_norm: called while a hipGraph is being captured -- the write would be replayed with "
                               "every step; call it before the capture or between replays")
        self.max_grad_norm = v
        if on and self._clip is not None:
            self._sync_clip()

    def _sync_clip(self):
        """the clip row exists and holds the host's max_norm (created / uploaded outside capture only)"""
        if self._clip is not None and self._clip_uploaded == self.max_grad_norm:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("AdamW: the clip row does not exist yet (or max_grad_norm changed on the host) and cannot be written while a "
                               "hipGraph is being captured; run one eager step before the capture")
        if self._clip is None:
            self._clip = grad_clip.new_row(self._device(), self.max_grad_norm)
        else:
            call("unetr_grad_clip_set", self._clip.data_ptr(), self.max_grad_norm, torch.cuda.current_stream().cuda_stream)
        self._clip_uploaded = self.max_grad_norm

    def _clip_row(self):
        if self.max_grad_norm is None:
            raise RuntimeError("AdamW was built without max_grad_norm: no gradient norm is measured")
        if self._clip is None:
            self._sync_clip()
        return self._clip

    def grad_norm(self):
        """the global gradient norm of the last step: a 0-d DEVICE view of the clip row (no synchronisation; ``float()`` it to read)"""
        return self._clip_row()[0]

    def clip_coef(self):
        """the factor the last step multiplied its gradients by, min(1, max_norm / (norm + 1e-6)): a 0-d device view"""
        return self._clip_row()[1]

    def nonfinite_steps(self):
        """how many steps so far had an inf / NaN gradient norm (a host read: it synchronises; meant for the end of an epoch)"""
        return int(self._clip_row()[3])

    def _gcoef_ptr(self):
        return self._clip.data_ptr() + 4

    def _clip_arena(self, pattern, src, gscale):
        """norm + coefficient of the gradients of ``pattern`` read from ``src``, a flat fp32 / bf16 tensor laid out like the arena (the
        gradient arena itself, or the all-reduced communication buffer: gscale = 1 / world): one table-driven launch + finalize"""
        self._sync_clip()
        ent = self._clip_tables.get(pattern)
        if ent is None:
            flat = self._flat
            table, nr, blocks = grad_clip.range_table(flat["offsets"], flat["params"], pattern, flat["param"].device)
            ent = self._clip_tables[pattern] = (table, nr, blocks, torch.zeros(max(blocks, 1), dtype=torch.float64, device=flat["param"].device))
        table, nr, blocks, ws = ent
        if not nr:
            return
        grad_clip.sumsq_ranges(src, table, nr, blocks, ws)
        grad_clip.finalize(ws, blocks, gscale, self._clip)

    def _clip_tensors(self, grads):
        """the same over a list of contiguous gradient tensors: one partial launch per tensor, each into its own workspace slots"""
        self._sync_clip()
        grads = [g for g in grads if g.numel()]
        need = sum(grad_clip.blocks_of(g.numel()) for g in grads)
        if not need:
            return
        if self._clip_ws is None or self._clip_ws.numel() < need:
            if self._clip_ws is not None:
                self._clip_ws_outgrown.append(self._clip_ws)      # (a captured step may still write the smaller one)
            self._clip_ws = torch.zeros(need, dtype=torch.float64, device=grads[0].device)
        grad_clip.finalize(self._clip_ws, grad_clip.sumsq_tensors(grads, self._clip_ws), 1.0, self._clip)

    def _adamw(self, p, g, g_bf16, gscale, m, v, n, gi, b1, b2, eps, step_ptr, sptr, wptr, stream):
        """one streaming AdamW launch; with clipping on, the form that also reads the coefficient of the clip row"""
        if self.max_grad_norm is None:
            call("unetr_adamw_hyper", p, g, g_bf16, gscale, m, v, n, self._hyper_ptr(gi), b1, b2, eps, step_ptr, sptr, wptr, stream)
        else:
            call("unetr_adamw_hyper_clip", p, g, g_bf16, gscale, m, v, n, self._hyper_ptr(gi), b1, b2, eps, step_ptr, sptr, wptr,
                 self._gcoef_ptr(), stream)

    # ---- checkpoints in torch.optim.AdamW's schema ------------------------------------------------------------------------
    def _arena_mode(self):
        """the moments live in the flat arenas (self.state stays empty: begin_fused_step relies on that)"""
        return self._flat is not None and not any(len(st) for st in self.state.values())

    @torch.no_grad()
    def state_dict(self):
        """``{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]}`` as torch.optim.AdamW writes it, for every
        parameter that has stepped -- in flat mode synthesised from the arenas (copies).  The groups also carry the schedule
        description and the group's step count ``t``.  Loads into torch.optim.AdamW over the same parameters, and back."""
        arena = self._arena_mode()
        state, groups, base = {}, [], 0
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            steps = self._steps[gi].cpu().tolist() if gi in self._steps else [0.0] * len(params)
            for i, p in enumerate(params):
                if steps[i] <= 0:
                    continue
                if arena:
                    if self._flat_state is None:
                        continue
                    o, n = self._flat["offsets"][i], p.numel()
                    m, v = (a[o:o + n].view(p.shape).clone() for a in self._flat_state)
                else:
                    st = self.state.get(p)
                    if not st:
                        continue
                    m, v = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
                state[base + i] = {"step": torch.tensor(float(steps[i]), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
            g = {k: v for k, v in group.items() if k != "params"}
            g.update({k: v for k, v in _TORCH_GROUP_KEYS.items() if k not in g})
            sched = self._schedule[gi] if gi < len(self._schedule) else None
            g["schedule"] = dict(sched[0]) if sched is not None else None
            g["t"] = int(self._hyper[gi, 2]) if self._hyper is not None else 0
            if sched is not None and self._hyper is not None and g["t"] > 0:
                g["lr"] = float(self._hyper[gi, 0])          # informational: the rate of the last step (the schedule recomputes it)
            g["params"] = list(range(base, base + len(params)))
            groups.append(g)
            base += len(params)
        return {"state": state, "param_groups": groups}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Load a dict written by ``state_dict()`` or by torch.optim.AdamW over the same parameters.  Everything is copied IN PLACE
        -- into the moment arenas (flat mode) or the existing per-tensor moments, the device step counters and the hyper rows --
        so graphs captured before the call stay valid; it may run before or after capture, not during one."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("AdamW.load_state_dict cannot run while a hipGraph is being captured")
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict has different param groups than this optimizer")
        if any(s.get("amsgrad") or s.get("maximize") for s in saved):
            raise ValueError("HIP AdamW has no amsgrad / maximize variant")
        if any(s.get("decoupled_weight_decay") is False for s in saved):
            raise ValueError("the loaded state belongs to Adam with coupled (L2) weight decay, not AdamW")
        arena = self._arena_mode()
        dev = self._device()
        # everything that can refuse is checked before the first byte is written
        plans = []
        for gi, (sg, group) in enumerate(zip(saved, self.param_groups)):
            entries = [state_dict["state"].get(k) for k in sg["params"]]
            steps = [float(e["step"]) if e else 0.0 for e in entries]
            for p, e in zip(group["params"], entries):
                if e and (tuple(e["exp_avg"].shape) != tuple(p.shape) or tuple(e["exp_avg_sq"].shape) != tuple(p.shape)):
                    raise ValueError("loaded optimizer state does not match the parameter shapes")
            if arena:
                for i, j in self._runs_captured:
                    if len(set(steps[i:j + 1])) > 1:
                        raise RuntimeError("load_state_dict: parameters that an already captured launch steps with ONE shared counter "
                                           f"(indices {i}..{j}) have different step counts in the loaded state")
            cur = self._schedule[gi][0] if self._schedule[gi] is not None else None
            desc = sg.get("schedule") if "schedule" in sg else cur       # (a dict from torch.optim.AdamW says nothing about schedules)
            if desc is not None:
                desc = dict(desc)
                if desc.get("kind") not in SCHEDULES:
                    raise ValueError(f"unknown schedule {desc.get('kind')!r} in the loaded state")
            if self._captured and desc != cur:
                raise RuntimeError("load_state_dict: the loaded schedule differs from the one frozen in an already captured step; "
                                   "attach it with set_schedule() before TrainStep captures")
            plans.append((entries, steps, desc))
        self.sync_hyper()          # (creates the rows)
        stream = torch.cuda.current_stream().cuda_stream
        for gi, (sg, group) in enumerate(zip(saved, self.param_groups)):
            entries, steps, desc = plans[gi]
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in sg:
                    group[k] = tuple(sg[k]) if k == "betas" else sg[k]
            if desc is not None:
                self._attach(gi, desc)
            elif self._schedule[gi] is not None:
                self._schedule[gi] = None
            params = group["params"]
            self._step_tensor(gi, dev).copy_(torch.tensor(steps, dtype=torch.float32))
            if arena:
                if self._flat_state is None:
                    self._flat_state = (torch.zeros_like(self._flat["param"]), torch.zeros_like(self._flat["param"]))
                m, v = self._flat_state
                m.zero_()
                v.zero_()
                for p, o, e in zip(params, self._flat["offsets"], entries):
                    if e:
                        m[o:o + p.numel()].copy_(e["exp_avg"].reshape(-1))
                        v[o:o + p.numel()].copy_(e["exp_avg_sq"].reshape(-1))
                self._host_steps = [int(t) for t in steps]
            else:
                for p, e in zip(params, entries):
                    st = self.state.get(p)
                    if not e:
                        if st:
                            st["exp_avg"].zero_()
                            st["exp_avg_sq"].zero_()
                        continue
                    if not st:
                        st = self.state[p]
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg"].copy_(e["exp_avg"])
                    st["exp_avg_sq"].copy_(e["exp_avg_sq"])
                if self._flat is not None:
                    self._host_steps = [int(t) for t in steps]
            # (a group never took fewer steps than one of its parameters: a dict that went through torch.optim.AdamW carries no
            # "t", or the one it was given when it loaded a dict of ours)
            t = max(float(sg.get("t", 0)), max(steps, default=0.0))
            call("unetr_adamw_hyper_set", self._hyper_ptr(gi), 4, 0.0, 0.0, t, stream)
        self.sync_hyper()          # the loaded lr / weight_decay

    def _advance_steps(self, gi, params, pattern, dev):
        self.sync_hyper()
        if torch.cuda.is_current_stream_capturing():
            self._captured = True
        steps = self._step_tensor(gi, dev)
        mask = self._masks.get((gi, pattern))
        if mask is None:
            mask = torch.tensor([1.0 if f else 0.0 for f in pattern], dtype=torch.float32, device=dev)
            self._masks[(gi, pattern)] = mask
        # one launch: the per-parameter counters, the group's step count t and -- with a schedule attached -- this step's lr
        sched = self._schedule[gi]
        call("unetr_counter_add_lr", steps.data_ptr(), mask.data_ptr(), steps.numel(), self._hyper_ptr(gi),
             ctypes.byref(sched[1]) if sched is not None else None, torch.cuda.current_stream().cuda_stream)
        return steps

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        stream = torch.cuda.current_stream().cuda_stream
        per_tensor = False
        contig = {}          # clipping, per-tensor path: the contiguous copies of non-contiguous gradients the norm was taken over
        if self.max_grad_norm is not None:
            # the norm is global over all groups and is taken before the first update
            group0 = self.param_groups[0]
            pattern0 = tuple(p.grad is not None for p in group0["params"])
            if self._flat is not None and any(pattern0) and self._grads_in_arena(group0["params"], pattern0):
                self._clip_arena(pattern0, self._flat["grad"], 1.0)
            else:
                grads = []
                for group in self.param_groups:
                    for p in group["params"]:
                        if p.grad is not None:
                            if not p.grad.is_cuda:
                                raise RuntimeError("HIP AdamW needs fp32 parameters on a ROCm device (no CPU fallback)")
                            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                            contig[id(p)] = g
                            grads.append(g)
                if grads:
                    self._clip_tensors(grads)
        for gi, group in enumerate(self.param_groups):
            b1, b2 = group["betas"]
            params = group["params"]
            pattern = tuple(p.grad is not None for p in params)
            if not any(pattern):
                continue
            dev = next(p for p in params if p.grad is not None).device
            if self._flat is not None and self._flat_step(group, params, pattern, dev, stream):
                continue
            per_tensor = True
            steps = self._advance_steps(gi, params, pattern, dev)
            for i, p in enumerate(params):
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError("HIP AdamW needs fp32 parameters on a ROCm device (no CPU fallback)")
                if not p.is_contiguous():
                    raise RuntimeError("HIP AdamW needs contiguous parameters")
                if not g.is_contiguous():
                    g = contig[id(p)] if id(p) in contig else g.contiguous()
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                self._adamw(p.data_ptr(), g.data_ptr(), 0, 1.0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                            gi, b1, b2, group["eps"], steps.data_ptr() + 4 * i, Fn.shadow_ptr_for_update(p), None, stream)
        if self._flat is not None and per_tensor:      # (per-tensor launches write neither the bf16x3 words nor the transposed twins)
            Fn.after_step(self._flat, [p for g in self.param_groups for p in g["params"] if p.grad is not None], arena=False, repack=False)
        Fn.refresh_conv_packs()          # one grouped launch: packed conv weights follow the update
        return loss

    def _flat_runs(self, params, pattern, max_elems=None, cuts=()):
        """Contiguous arena ranges (i, j, lo, hi) of parameters that step together: consecutive parameters with a
        gradient and equal step counts, optionally cut at parameter boundaries into pieces of <= max_elems and at the
        arena offsets listed in ``cuts`` (the boundaries of the data-parallel communication pieces)."""
        offs = self._flat["offsets"]
        cuts = set(cuts)
        runs, i, n = [], 0, len(params)
        while i < n:
            if not pattern[i]:
                i += 1
                continue
            j = i
            while (j + 1 < n and pattern[j + 1] and self._host_steps[j + 1] == self._host_steps[i]
                   and offs[j + 1] not in cuts and (max_elems is None or offs[j + 1] + params[j + 1].numel() - offs[i] <= max_elems)):
                j += 1
            runs.append((i, j, offs[i], offs[j] + (params[j].numel() + 3) // 4 * 4))
            i = j + 1
        return runs

    def _launch_run(self, group, run, steps, gptr, g_bf16, gscale, stream):
        flat = self._flat
        i, j, lo, hi = run
        m, v = self._flat_state
        b1, b2 = group["betas"]
        shadow = flat.get("shadow")            # bf16 copy of the arena read by the bf16-storage GEMMs, refreshed in the same kernel
        sptr = shadow.data_ptr() + lo * 2 if shadow is not None else None
        words = flat.get("shadow_x3")          # bf16x3 mode: the word shadow (derived_weights.weight_x3), written by the same kernel
        wptr = words.data_ptr() + lo * 4 if words is not None else None
        self._adamw(flat["param"].data_ptr() + lo * 4, gptr + lo * (2 if g_bf16 else 4), int(g_bf16), gscale,
                    m.data_ptr() + lo * 4, v.data_ptr() + lo * 4, hi - lo, 0, b1, b2, group["eps"],
                    steps.data_ptr() + 4 * i, sptr, wptr, stream)
        if torch.cuda.is_current_stream_capturing():
            self._runs_captured.add((i, j))
        for k in range(i, j + 1):
            self._host_steps[k] += 1

    def _grads_in_arena(self, params, pattern):
        gbase = self._flat["grad"].data_ptr()
        return all(not has or p.grad.data_ptr() == gbase + o * 4 for p, o, has in zip(params, self._flat["offsets"], pattern))

    def _flat_step(self, group, params, pattern, dev, stream):
        """One launch per contiguous run of parameters with arena gradients and equal step counts."""
        flat = self._flat
        gbase = flat["grad"].data_ptr()
        if not self._grads_in_arena(params, pattern):
            return False          # some gradient is not in the arena (e.g. accumulated): per-tensor path
        if self._flat_state is None:
            self._flat_state = (torch.zeros_like(flat["param"]), torch.zeros_like(flat["param"]))
        steps = self._advance_steps(0, params, pattern, dev)
        for run in self._flat_runs(params, pattern):
            self._launch_run(group, run, steps, gbase, False, 1.0, stream)
        Fn.after_step(flat, [p for p, has in zip(params, pattern) if has], arena=True, repack=False)      # (step() re-packs once, at its end)
        return True

    # ---- single-GPU fused step: AdamW of the ViT Linear weights rides on the grouped weight-gradient launch ----------------
    # begin_fused_step(pattern) AFTER the forward and BEFORE backward (step counters advance, the arena state is handed to
    # functional.flush_deferred; the model's next forward drops an arming whose step never finished),
    # finish_fused_step() AFTER backward: one table-driven launch updates every parameter the fused launch did not cover.
    # The gradients of the fused weights are never written: p.grad of those parameters names a stale arena slice.
    @torch.no_grad()
    def begin_fused_step(self, pattern):
        from . import _capi
        flat = self._flat
        if self.max_grad_norm is not None:
            raise RuntimeError("begin_fused_step: gradient clipping (max_grad_norm) cannot be combined with the fused update -- the "
                               "weight-gradient epilogue updates the ViT weights inside the launch that produces their gradients, when "
                               "no global gradient norm exists yet; use the unfused step")
        if flat is None or len(self.param_groups) != 1 or flat.get("state") is None:
            raise RuntimeError("begin_fused_step needs AdamW(..., flat=model.use_flat_buffers())")
        group = self.param_groups[0]
        params = group["params"]
        pattern = tuple(bool(f) for f in pattern)
        # everything that can be checked BEFORE backward is checked here: the epilogue updates the ViT weights during backward,
        # so a failure found afterwards (finish_fused_step) leaves the model half-updated
        for p, has in zip(params, pattern):
            if has and p.grad is not None:
                raise RuntimeError("fused step: a planned parameter already carries .grad (its gradient would be accumulated outside "
                                   "the arena); call zero_grad(set_to_none=True) before the step")
            if self.state.get(p):
                raise RuntimeError("fused step: this optimizer has per-tensor AdamW state (an earlier step() took the per-tensor path); "
                                   "the arena moments would silently restart from zero")
        if self._flat_state is None:
            self._flat_state = (torch.zeros_like(flat["param"]), torch.zeros_like(flat["param"]))
        steps = self._advance_steps(0, params, pattern, flat["param"].device)
        m, v = self._flat_state
        shadow = flat.get("shadow")
        b1, b2 = group["betas"]
        words = flat.get("shadow_x3")
        arena = _capi.AdamWArena(flat["param"].data_ptr(), flat["grad"].data_ptr(), m.data_ptr(), v.data_ptr(),
                                 shadow.data_ptr() if shadow is not None else None, steps.data_ptr(), flat["param"].numel(),
                                 group["lr"], b1, b2, group["eps"], group["weight_decay"], words.data_ptr() if words is not None else None,
                                 self._hyper_ptr(0))      # (the kernels read lr / weight_decay from the row; the by-value fields are not used)
        gbase = flat["grad"].data_ptr()
        index = {gbase + o * 4: i for i, (o, has) in enumerate(zip(flat["offsets"], pattern)) if has}
        self._fused = dict(pattern=pattern, arena=arena, index=index, done=[], keep=(m, v, steps), flat=flat, wt_done=[])
        flat["state"].fuse = self._fused

    @torch.no_grad()
    def finish_fused_step(self):
        """A RuntimeError raised here is fatal for the step: the weight-gradient epilogue has already updated the fused weights
        and the step counters have advanced, the remaining parameters have not stepped -- reload a checkpoint."""
        import ctypes
        flat, fz = self._flat, self._fused
        flat["state"].fuse = None
        self._fused = None
        group = self.param_groups[0]
        params = group["params"]
        pattern = fz["pattern"]
        if tuple(p.grad is not None for p in params) != pattern:
            raise RuntimeError("fused step: the set of parameters that received gradients differs from the planned pattern")
        gbase = flat["grad"].data_ptr()
        done = set(fz["done"])
        self.fused_parameters = len(done)          # how many parameters the weight-gradient launch updated itself in this step
        for i, (p, o, has) in enumerate(zip(params, flat["offsets"], pattern)):
            if has and i not in done and p.grad.data_ptr() != gbase + o * 4:
                raise RuntimeError("fused step: a gradient was produced outside the arena")
        rest = tuple(has and i not in done for i, has in enumerate(pattern))
        # a run shares ONE step counter (its first parameter's): the runs depend on which neighbours have equal step counts, so
        # their boundaries are part of the key (alternating patterns -- the feat / recon passes of the ranking pre-training --
        # make counts diverge between two uses of the same pattern)
        runs = self._flat_runs(params, rest)
        if torch.cuda.is_current_stream_capturing():
            self._runs_captured.update((i, j) for i, j, _, _ in runs)
        key = (pattern, tuple(sorted(done)), tuple((i, j) for i, j, _, _ in runs))
        cache = getattr(self, "_range_tables", None)
        if cache is None:
            cache = self._range_tables = {}
        ent = cache.get(key)
        if ent is None:
            rows, blocks = [], 0
            for i, j, lo, hi in runs:
                rows.append((lo, hi, i, blocks))
                blocks += (hi - lo + 4095) // 4096
            table = torch.tensor(rows, dtype=torch.int64, device=flat["param"].device) if rows else None
            ent = cache[key] = (table, len(rows), blocks)
        table, nr, blocks = ent
        if nr:
            call("unetr_adamw_ranges", ctypes.byref(fz["arena"]), table.data_ptr(), nr, blocks, torch.cuda.current_stream().cuda_stream)
        for k, has in enumerate(pattern):
            if has:
                self._host_steps[k] += 1
        Fn.after_step(flat, [p for p, has in zip(params, pattern) if has], arena=True, twins_written=[params[i] for i in fz["wt_done"]])

    # ---- data-parallel arena update: all-reduce pieces overlap the optimizer kernels of the pieces before them ----
    def plan_reduced(self, max_elems=None, cuts=(), pattern=None):
        """Freeze a gradient pattern (default: which parameters have .grad now) into arena ranges of <= max_elems that never
        straddle an offset in ``cuts``.  The plan is reused every step by ``step_reduced`` / ``step_runs`` -- under hipGraph
        replay ``.grad`` attributes do not change."""
        if self._flat is None or len(self.param_groups) != 1:
            raise RuntimeError("plan_reduced needs AdamW(..., flat=model.use_flat_buffers())")
        params = self.param_groups[0]["params"]
        pattern = tuple(p.grad is not None for p in params) if pattern is None else tuple(bool(f) for f in pattern)
        return dict(pattern=pattern, runs=self._flat_runs(params, pattern, max_elems, cuts))

    # ---- the reduced step in pieces (train_step.TrainStep, data-parallel form): begin -> step_runs per piece -> end, each on
    # whatever stream is current (the communication stream, right behind the piece's all-reduce)
    @torch.no_grad()
    def begin_reduced_step(self, plan):
        if self._flat_state is None:
            self._flat_state = (torch.zeros_like(self._flat["param"]), torch.zeros_like(self._flat["param"]))
        return self._advance_steps(0, self.param_groups[0]["params"], plan["pattern"], self._flat["param"].device)

    @torch.no_grad()
    def clip_reduced(self, plan, gsrc, gscale):
        """Clipping on: norm and coefficient of the planned gradients read from ``gsrc`` (the communication buffer once EVERY piece
        has been reduced) times ``gscale``, on the current stream.  ``step_runs`` must follow it, not precede it: every rank measures
        the same reduced buffer and gets the same coefficient.  A no-op when clipping is off."""
        if self.max_grad_norm is not None:
            self._clip_arena(plan["pattern"], gsrc, gscale)

    @torch.no_grad()
    def step_runs(self, plan, ks, steps, gsrc, gscale):
        g_bf16 = gsrc.dtype == torch.bfloat16
        if not g_bf16 and gsrc.dtype != torch.float32:
            raise RuntimeError("gradient source must be fp32 or bf16")
        stream = torch.cuda.current_stream().cuda_stream
        for k in ks:
            self._launch_run(self.param_groups[0], plan["runs"][k], steps, gsrc.data_ptr(), g_bf16, gscale, stream)

    @torch.no_grad()
    def end_reduced_step(self, plan):
        Fn.after_step(self._flat, [p for p, has in zip(self._flat["params"], plan["pattern"]) if has], arena=True)

    @torch.no_grad()
    def step_reduced(self, plan, gsrc, gscale, before_run=None, order=None):
        """AdamW over the planned ranges with gradients read from ``gsrc`` (a flat fp32 or bf16 tensor laid out like
        the arena: the all-reduced communication buffer) times ``gscale``.  ``before_run(k, lo, hi)`` runs before range
        k's kernel is launched -- the caller makes the current stream wait for that range's all-reduce there."""
        group = self.param_groups[0]
        stream = torch.cuda.current_stream().cuda_stream
        steps = self.begin_reduced_step(plan)
        g_bf16 = gsrc.dtype == torch.bfloat16
        if not g_bf16 and gsrc.dtype != torch.float32:
            raise RuntimeError("gradient source must be fp32 or bf16")
        runs = plan["runs"]
        order = list(order if order is not None else range(len(runs)))      # order: the order the pieces finish reducing in
        if self.max_grad_norm is not None:
            # the global norm needs every range reduced: all the waits first, then the norm, then the updates
            if before_run is not None:
                for k in order:
                    before_run(k, runs[k][2], runs[k][3])
            before_run = None
            self.clip_reduced(plan, gsrc, gscale)
        for k in order:
            run = runs[k]
            if before_run is not None:
                before_run(k, run[2], run[3])
            self._launch_run(group, run, steps, gsrc.data_ptr(), g_bf16, gscale, stream)
        self.end_reduced_step(plan)
