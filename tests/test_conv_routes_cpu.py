"""Host logic of the conv side of functional.py on CPU tensors: which kernels ResBlockFn, TconvFn, UpBlockFn, OutConvFn and the public
wrappers launch, in which order and with which arguments, on every route -- the fused forms, each fallback a kernel's "unsupported"
answer leads to, the generic im2col family, arena mode and its queued reductions.  Most fallbacks are never reached by a GPU test at real
shapes (the dedicated kernels accept those), so a comparison of results would not notice one that changed.

The seams are those of tests/test_derived_weights_cpu.py: the ABI `call` / `call_rc`, the stream lookup, the workspace, the device check,
the library handle, the capture query and the pack-size query are replaced; no kernel runs.  Every launch is logged with all its
arguments: structs field by field, pointers as `label+byte offset` into the scenario's named tensors, the workspace, or the tensors the
code under test allocated (a0, a1, ... in allocation order, all kept alive so that no address repeats).  A pointer into none of them --
the result of a torch cast on a generic-family boundary -- is logged as `other`.

The expected logs (tests/conv_routes_parent_log.json) were NOT taken from the code under test: this driver was run against an untouched
checkout of commit dd787cc ("Add a fused segmentation loss family"), the parent of the change that gave the block routes one result shape
each, and what it printed was committed: for every scenario the number of log entries and a digest of them, and for a few
representative scenarios (FULL) the whole log.  To print the same of any checkout:  python tests/test_conv_routes_cpu.py <checkout>
(with --full: every entry of every scenario, one per line, for a diff between two trees)."""
import ctypes
import hashlib
import importlib
import json
import os
import sys

import pytest
import torch

STREAM = 77
ROWS_OUT = 2          # what a kernel reports through a c_int / c_long out-parameter
ROWS_QUERY = 3        # what the library's *_rows queries answer
ENV = ("UNETR_AMD_IN_FUSE", "UNETR_AMD_OUT_FUSE")
LOG_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_routes_parent_log.json")


class TorchProxy:
    """`torch` as the modules under test see it: the allocating calls hand their tensors to the world, which labels them"""

    def __init__(self, world):
        self._world = world

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **k):
        return self._world.allocated(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._world.allocated(torch.empty_like(*a, **k))

    def zeros(self, *a, **k):
        return self._world.allocated(torch.zeros(*a, **k))


class World:
    """one scenario: the seams, the named tensors, the log"""

    def __init__(self, pkg, mp, prec, decline=None, rows=None, env=None, arena=False):
        self.pkg, self.mp, self.prec, self.arena = pkg, mp, prec, arena
        self.Fn, self.capi = pkg.functional, pkg._capi
        self.decline = decline or {}       # kernel name -> True (always) or the set of its calls, counted from 1, that answer "unsupported"
        self.rows = rows or {}             # *_rows query -> answer (default ROWS_QUERY)
        self.count, self.known, self.nalloc, self.log, self.st = {}, [], 0, [], None
        self.ws = self.know("ws", torch.zeros(4096))
        self.install(env or {})

    # ---- the seams (they and this driver are all that may differ between the run at the parent and the run at the change) ----
    def install(self, env):
        Fn, dw, ga, mp = self.Fn, self.pkg.derived_weights, self.pkg.grad_arena, self.mp
        proxy = TorchProxy(self)
        for mod in (Fn, dw, ga):
            mp.setattr(mod, "call", self.call)
            mp.setattr(mod, "_stream", lambda: STREAM)
            mp.setattr(mod, "torch", proxy)
        mp.setattr(Fn, "call_rc", self.call_rc)
        mp.setattr(Fn, "workspace", lambda device: self.ws)
        mp.setattr(Fn, "_require_gpu", lambda *a, **k: None)
        mp.setattr(self.capi, "load", lambda: self)          # (the *_rows queries: __getattr__ below)
        mp.setattr(dw, "_capturing", lambda: False)
        mp.setattr(dw, "_pack_bytes", lambda w, kind, prec: 64 + 16 * kind + 8 * prec)
        for kind in (dw.BF16, dw.WORDS, dw.TWIN, dw.PACK):
            mp.setattr(kind, "table", {})
            mp.setattr(kind, "by_addr", {})
        for name in ENV:
            if name in env:
                mp.setenv(name, env[name])
            else:
                mp.delenv(name, raising=False)

    def __getattr__(self, name):
        if not name.endswith("_rows"):
            raise AttributeError(name)

        def query(*args):
            self.log.append(["query " + name] + list(args))
            return self.rows.get(name, ROWS_QUERY)
        return query

    def close(self):
        if self.st is not None:
            self.pkg.grad_arena.clear_grad_sinks(self.st)

    # ---- tensors ----
    def know(self, label, t):
        st = t.untyped_storage()
        self.known = [k for k in self.known if k[1] != st.data_ptr()] + [(label, st.data_ptr(), st.nbytes(), t)]
        return t

    def allocated(self, t):
        self.nalloc += 1
        return self.know(f"a{self.nalloc - 1}", t)

    def adt(self):
        return torch.bfloat16 if self.prec == 1 else torch.float32

    def input(self, label, shape, dtype=None, grad=True):
        t = self.know(label, torch.zeros(*shape, dtype=dtype or self.adt()))
        return t.requires_grad_() if grad else t

    def weights(self, **shapes):
        """parameters of the given shapes: on their own, or (arena mode) in flat arenas registered with one ArenaState"""
        if not self.arena:
            return [self.know(k, torch.nn.Parameter(torch.zeros(s))) for k, s in shapes.items()]
        ga = self.pkg.grad_arena
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes.values()]
        offs, n = [], 0
        for p in ps:
            offs.append(n)
            n += (p.numel() + 7) // 8 * 8
        param, grad = self.know("param", torch.zeros(n)), self.know("grad", torch.zeros(n))
        views = []
        for p, o in zip(ps, offs):
            p.data = param[o:o + p.numel()].view_as(p)
            views.append((p, grad[o:o + p.numel()].view_as(p)))
        self.st = ga.register_grad_sinks(views, ga.ArenaState())
        return ps

    # ---- the log ----
    def ptr(self, v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if v is None:
            return None
        if v == STREAM:
            return "stream"
        for label, base, nbytes, _ in self.known:
            if base <= v < base + max(1, nbytes):
                return f"{label}+{v - base}"
        return "other"

    def struct(self, s):
        return {f: self.ptr(getattr(s, f)) if t is ctypes.c_void_p else self.plain(getattr(s, f)) for f, t in s._fields_}

    def plain(self, a):
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:          # (the prefetch descriptor's pointers)
                return [self.ptr(e) for e in a]
            return [self.struct(e) if isinstance(e, ctypes.Structure) else e for e in a]
        if isinstance(a, ctypes.Structure):
            return self.struct(a)
        return a

    def show(self, a, argtype):
        if argtype is ctypes.c_void_p:
            return self.ptr(a)
        if hasattr(a, "_obj"):          # ctypes.byref
            return self.struct(a._obj) if isinstance(a._obj, ctypes.Structure) else "out"
        return self.plain(a)

    def call(self, name, *args):
        sig = self.capi._SIGNATURES[name]
        assert len(sig) == len(args), name
        self.log.append([name] + [self.show(a, t) for a, t in zip(args, sig)])

    def call_rc(self, name, *args):
        self.call(name, *args)
        n = self.count[name] = self.count.get(name, 0) + 1
        rule = self.decline.get(name)
        if rule is True or (rule and n in rule):
            self.log.append(["-> unsupported"])
            return 3
        for a in args:
            if hasattr(a, "_obj") and isinstance(a._obj, (ctypes.c_int, ctypes.c_long)):
                a._obj.value = ROWS_OUT
        return 0

    def tensor(self, t):
        """a result: where it lives, shape, strides, type"""
        return None if t is None else [self.ptr(t.data_ptr()), list(t.shape), list(t.stride()), str(t.dtype)]

    def note(self, what, *vals):
        self.log.append([what] + list(vals))

    def forward(self, fn, *args):
        out = fn.apply(*args)
        self.note("forward ->", self.tensor(out))
        return out

    def backward(self, out, **wrt):
        """one real backward pass from a named zero gradient; then what each input and parameter received (a parameter of an arena:
        the slice attached as .grad; anything else went through autograd's own accumulation: shape and type only)"""
        dout = self.know("dout", torch.zeros(out.shape, dtype=out.dtype))
        self.note("backward")
        torch.autograd.backward([out], [dout])
        self.grads(**wrt)

    def grads(self, **wrt):
        got = {}
        for k, t in wrt.items():
            g = t.grad
            where = None if g is None else self.ptr(g.data_ptr())
            got[k] = None if g is None else [where if where.startswith("grad+") else "-", list(g.shape), str(g.dtype)]
        self.note("grads", got)


# ------------------------------------------------------------------------------------------------------------------ scenarios
F32 = torch.float32


def resblock(W, cin=16, cout=16, image=False, to_cat=False, need_dx=True):
    B, D, H, Wd = 2, 2, 2, 3
    x = W.input("x", (B, D, H, Wd, cin), F32 if image else None, grad=need_dx and not image)
    w1, w2, w3 = W.weights(w1=(cout, cin, 3, 3, 3), w2=(cout, cout, 3, 3, 3), w3=(cout, cin, 1, 1, 1))
    out = W.forward(W.Fn.ResBlockFn, x, w1, w2, w3, W.prec, to_cat)
    W.backward(out, x=x, w1=w1, w2=w2, w3=w3)


def tconv(W, cin=8, cout=4, tokens=False, to_cat=False, need_dx=True, B=1):
    x = W.input("x", (B, 2, 2, 2, cin), F32 if tokens else None, grad=need_dx)
    w, = W.weights(w=(cin, cout, 2, 2, 2))
    out = W.forward(W.Fn.TconvFn, x, w, W.prec, to_cat)
    W.backward(out, x=x, w=w)


def upblock(W, head=False, skip="copy", cin=8, C=16, inp_grad=True, sp=(1, 1, 2)):
    Fn, B, (D, H, Wd) = W.Fn, 1, sp
    inp = W.input("inp", (B, D, H, Wd, cin), grad=inp_grad)
    shapes = dict(wt=(cin, C, 2, 2, 2), w1=(C, 2 * C, 3, 3, 3), w2=(C, C, 3, 3, 3), w3=(C, 2 * C, 1, 1, 1))
    if head:
        shapes.update(wo=(3, C, 1, 1, 1), bo=(3,))
    if skip == "chain":
        shapes.update(ws=(cin, C, 2, 2, 2))
    ps = dict(zip(shapes, W.weights(**shapes)))
    leaves = dict(inp=inp, **ps)
    if skip == "chain":          # the skip tensor as its producer leaves it: the second half of a fresh concatenation buffer
        leaves["xs"] = W.input("xs", (B, D, H, Wd, cin))
        sk = W.forward(Fn.TconvFn, leaves["xs"], ps["ws"], W.prec, True)
    else:
        sk = leaves["skip"] = W.input("skip", (B, 2 * D, 2 * H, 2 * Wd, C), F32 if skip == "fp32" else None)
    args = (inp, sk, ps["wt"], ps["w1"], ps["w2"], ps["w3"], W.prec, skip in ("chain", "refuse")) + ((ps["wo"], ps["bo"]) if head else ())
    if skip == "refuse":
        with pytest.raises(RuntimeError, match="skip_half"):
            Fn.UpBlockFn.apply(*args)
        return W.note("refused")
    out = W.forward(Fn.UpBlockFn, *args)
    W.backward(out, **leaves)


def outconv(W):
    x = W.input("x", (1, 2, 2, 2, 16))
    w, b = W.weights(w=(3, 16, 1, 1, 1), b=(3,))
    out = W.forward(W.Fn.OutConvFn, x, w, b)
    W.backward(out, x=x, w=w, b=b)


def wrappers(W):
    """the public wrappers that tests and tools call directly, on contiguous rows and on the halves of wider buffers"""
    Fn, prec, adt = W.Fn, W.prec, W.adt()
    B, D, H, Wd, V = 1, 2, 2, 2, 8
    dims = (B, D, H, Wd)

    def rows(label, c, dtype=adt, pitch=1, spatial=(D, H, Wd)):
        t = W.know(label, torch.zeros(B, *spatial, pitch * c, dtype=dtype))
        return t[..., c:] if pitch > 1 else t

    def shown(r):
        return [W.tensor(t) if isinstance(t, torch.Tensor) else t for t in r] if isinstance(r, (tuple, list)) else (W.tensor(r) if isinstance(r, torch.Tensor) else r)

    def step(name, r):
        W.note(name + " ->", shown(r))
    w = W.know("w", torch.zeros(16, 8, 3, 3, 3))
    w3 = W.know("w3", torch.zeros(16, 8, 1, 1, 1))
    ww = W.know("ww", torch.zeros(16, 16, 3, 3, 3))
    wg = W.know("wg", torch.zeros(4, 8, 3, 3, 3))          # cout % 16 != 0: the generic family
    wbig = W.know("wbig", torch.zeros(144, 8, 3, 3, 3))
    x, xv = rows("x", 8), rows("xv", 8, pitch=2)
    c, c3 = rows("c", 16), rows("c3", 16)
    half = rows("cat", 16, pitch=2)
    step("conv3", Fn.conv3(x, 8, w, dims, prec))
    step("conv3 view", Fn.conv3(xv, 16, w, dims, prec))
    step("conv3 dgrad into half, accumulate", Fn.conv3(c, 16, ww, dims, prec, mode=1, out=half, ldo=32, accumulate=True))
    step("conv3 generic", Fn.conv3(x, 8, wg, dims, prec))
    step("conv3 generic view", Fn.conv3(xv, 16, wg, dims, prec))
    step("conv3 generic dgrad, accumulate", Fn.conv3(rows("g4", 4), 4, wg, dims, prec, mode=1, out=rows("dx8", 8), ldo=8, accumulate=True))
    step("conv3_fused", Fn.conv3_fused(x, 8, w, w3, dims, prec))
    step("conv3_fused, no w3", Fn.conv3_fused(xv, 16, w, None, dims, prec))
    step("conv3_fused, image", Fn.conv3_fused(rows("img8", 8, F32), 8, w, w3, dims, prec))
    step("conv3_fused, cout 4", Fn.conv3_fused(x, 8, wg, None, dims, prec))
    step("conv3_parts", Fn.conv3_parts(x, 8, w, w3, dims, prec))
    step("conv3_parts, store3=False", Fn.conv3_parts(xv, 16, w, w3, dims, prec, store3=False))
    step("conv3_parts, no w3", Fn.conv3_parts(x, 8, w, None, dims, prec))
    step("conv3_parts, cout 144", Fn.conv3_parts(x, 8, wbig, None, dims, prec))
    part = W.know("part", torch.zeros(B, 1024, 2, 16))
    part_b = W.know("part_b", torch.zeros(B, 1024, 2, 16))
    part3 = W.know("part3", torch.zeros(B, 4, 3, 16))
    sa, sb = W.know("sa", torch.zeros(B, 16, 2)), W.know("sb", torch.zeros(B, 16, 2))
    step("instnorm_stats", Fn.instnorm_stats(half, 32, B, V, 16))
    step("instnorm_apply", Fn.instnorm_apply(c, sa, B, V, 16, True))
    step("instnorm_apply dual into half", Fn.instnorm_apply(c, sa, B, V, 16, True, x2=c3, sb=sb, out=half, ldo=32))
    step("instnorm_apply_fin", Fn.instnorm_apply_fin(c, part, 2, B, V, 16, True))
    step("instnorm_apply_fin dual into half", Fn.instnorm_apply_fin(c, part, 2, B, V, 16, True, x2=c3, part_b=part_b, rows_b=3, out=half, ldo=32))
    img = rows("img", 4, F32)
    w3i = W.know("w3i", torch.zeros(16, 4, 1, 1, 1))
    step("instnorm_apply_fin_img", Fn.instnorm_apply_fin_img(c, part, 2, img, 4, w3i, part_b, 3, B, V, 16))
    step("instnorm_apply_fin_img into half", Fn.instnorm_apply_fin_img(c, part, 2, img, 4, w3i, part_b, 3, B, V, 16, out=half, ldo=32))
    dy = rows("dy", 16)
    dy32 = rows("dy32", 16, torch.bfloat16 if adt is F32 else F32)        # a gradient in the other storage type: cast at the door
    step("instnorm_bwd", Fn.instnorm_bwd(half, 32, c, sa, B, V, 16, True))
    step("instnorm_bwd dual", Fn.instnorm_bwd(dy, 16, c, sa, B, V, 16, True, x2=c3, sb=sb))
    step("instnorm_bwd other type", Fn.instnorm_bwd(dy32, 16, c, sa, B, V, 16, False))
    step("instnorm_bwd_img", Fn.instnorm_bwd_img(half, 32, c, sa, img, 4, w3i, sb, B, V, 16))
    step("instnorm_bwd_img other type", Fn.instnorm_bwd_img(dy32, 16, c, sa, img, 4, w3i, sb, B, V, 16))
    step("instnorm_bwd_apply_fin", Fn.instnorm_bwd_apply_fin(half, 32, c, sa, part, 2, 2, B, V, 16, True))
    step("instnorm_bwd_apply_fin_dual", Fn.instnorm_bwd_apply_fin_dual(dy, 16, c, sa, c3, sb, part3, 4, B, V, 16))
    step("conv3_dgrad_stats", Fn.conv3_dgrad_stats(dy, ww, c, sa, dims, prec))
    step("conv3_dgrad_stats, pitched xn", Fn.conv3_dgrad_stats(dy, ww, half, sa, dims, prec))
    step("conv3_dgrad_fused", Fn.conv3_dgrad_fused(dy, c3, W.know("w16", torch.zeros(16, 16, 3, 3, 3)), W.know("w316", torch.zeros(16, 16, 1, 1, 1)),
                                                  rows("dx16", 16), dims, prec))
    step("conv3_dgrad_fused, cin 8", Fn.conv3_dgrad_fused(dy, c3, w, w3, rows("dx8b", 8), dims, prec))
    step("conv3_wgrad", Fn.conv3_wgrad(xv, 16, dy, 16, dims, 8, 16, prec))
    step("conv3_wgrad with 1x1", Fn.conv3_wgrad(x, 8, dy, 16, dims, 8, 16, prec, out=W.know("dw", torch.zeros(16, 8, 3, 3, 3)), dy3=c3,
                                               out3=W.know("dw3", torch.zeros(16, 8, 1, 1, 1))))
    pk = Fn.conv_pack(wg, 0)
    step("conv_pack", pk)
    for ks, pack in ((3, pk), (1, Fn.conv_pack(w3, 0))):
        co = 4 if ks == 3 else 16
        step(f"conv_fwd ks{ks}", Fn.conv_fwd(x, 8, pack, dims, 8, co, ks, prec))
        step(f"conv_fwd ks{ks} view", Fn.conv_fwd(xv, 16, pack, dims, 8, co, ks, prec))
        o = rows(f"o{ks}", co, pitch=2)
        step(f"conv_fwd ks{ks} into half", Fn.conv_fwd(x, 8, pack, dims, 8, co, ks, prec, out=o, ldo=2 * co))
        step(f"conv_fwd ks{ks} accumulate", Fn.conv_fwd(x, 8, pack, dims, 8, co, ks, prec, out=rows(f"oc{ks}", co), ldo=co, accumulate=True))
        g = rows(f"g{ks}", co)
        step(f"conv_wgrad ks{ks}", Fn.conv_wgrad(x, 8, g, co, dims, 8, co, ks, prec))
        step(f"conv_wgrad ks{ks} view, out", Fn.conv_wgrad(xv, 16, g, co, dims, 8, co, ks, prec, out=W.know(f"dwg{ks}", torch.zeros(co, 8, ks, ks, ks))))
    # transposed conv: contiguous rows and halves, with the dedicated kernels accepting and declining (the scenario's decline set)
    wt = W.know("wt", torch.zeros(8, 4, 2, 2, 2))
    dyt, dytv = rows("dyt", 4, spatial=(4, 4, 4)), rows("dytv", 4, pitch=2, spatial=(4, 4, 4))
    step("tconv_fwd", Fn.tconv_fwd(x, 8, wt, dims, 8, 4, prec))
    step("tconv_fwd view into half", Fn.tconv_fwd(xv, 16, wt, dims, 8, 4, prec, out=rows("tcat", 4, pitch=2, spatial=(4, 4, 4)), ldo=8))
    step("tconv_fwd tokens", Fn.tconv_fwd(rows("tok", 8, F32), 8, wt, dims, 8, 4, prec))
    step("tconv_dgrad", Fn.tconv_dgrad(dyt, 4, wt, dims, 8, 4, prec))
    step("tconv_dgrad view", Fn.tconv_dgrad(dytv, 8, wt, dims, 8, 4, prec))
    step("tconv_wgrad", Fn.tconv_wgrad(x, 8, dyt, 4, dims, 8, 4, prec))
    step("tconv_wgrad views, out", Fn.tconv_wgrad(xv, 16, dytv, 8, dims, 8, 4, prec, out=W.know("dwt", torch.zeros(8, 4, 2, 2, 2))))
    step("tconv_bwd", Fn.tconv_bwd(xv, 16, None, dytv, 8, wt, dims, 8, 4, prec, True))
    step("tconv_bwd tokens, other type", Fn.tconv_bwd(rows("tok2", 8, F32), 8, None, rows("dyt32", 4, F32, spatial=(4, 4, 4)), 4, wt, dims, 8, 4, prec, False))
    step("skip_half", Fn.skip_half(dims, 16, prec, x.device))
    step("outconv_in_fwd", Fn.outconv_in_fwd(c, part, 2, c3, part_b, 3, W.know("wo", torch.zeros(3, 16, 1, 1, 1)), W.know("bo", torch.zeros(3)), B, V, 16))
    step("outconv_in_fwd, wrong width", Fn.outconv_in_fwd(c, part, 2, c3, part_b, 3, w3, None, B, V, 16))
    step("levels", [Fn.in_fuse_level(), Fn.out_fuse_enabled()])


TCONV2 = ("unetr_tconv2_fwd", "unetr_tconv2_dgrad", "unetr_tconv2_wgrad")
TCONV2_ARENA = TCONV2 + ("unetr_tconv2_wgrad_parts",)
CASES = {}


def case(name, fn, precs=(0, 1, 2), **opt):
    world = {k: opt.pop(k) for k in ("decline", "rows", "env", "arena") if k in opt}
    for prec in precs:
        CASES[f"{name} p{prec}"] = (fn, prec, world, opt)


def both(name, fn, **opt):
    """a scenario with no arena and with its parameters in one"""
    case(name, fn, **opt)
    case(name + " arena", fn, arena=True, **opt)


# -- the residual block on a feature map, cout % 16 == 0
both("res", resblock)
for level in "012":
    both(f"res IN_FUSE={level}", resblock, env={"UNETR_AMD_IN_FUSE": level})
case("res OUT_FUSE=0", resblock, env={"UNETR_AMD_OUT_FUSE": "0"})
case("res to_cat", resblock, to_cat=True)
case("res to_cat IN_FUSE=0", resblock, to_cat=True, env={"UNETR_AMD_IN_FUSE": "0"})
both("res no dx", resblock, need_dx=False)
both("res cin 8", resblock, cin=8)                  # the input gradient takes the two-kernel route
case("res arena, no partial rows", resblock, arena=True, rows={"unetr_conv3_wgrad_rows": 0})
# -- on the image
for ci in (1, 4):
    both(f"img{ci}", resblock, image=True, cin=ci)
    case(f"img{ci} to_cat", resblock, image=True, cin=ci, to_cat=True)
    case(f"img{ci} IN_FUSE=0", resblock, image=True, cin=ci, env={"UNETR_AMD_IN_FUSE": "0"})
    case(f"img{ci} parts declines once", resblock, image=True, cin=ci, decline={"unetr_conv3_fwd_parts": {1}})
    case(f"img{ci} parts declines", resblock, image=True, cin=ci, decline={"unetr_conv3_fwd_parts": True})
    both(f"img{ci} apply_fin_img declines", resblock, image=True, cin=ci, decline={"unetr_instnorm_apply_fin_img": True})
    case(f"img{ci} apply_fin_img declines, to_cat", resblock, image=True, cin=ci, to_cat=True, decline={"unetr_instnorm_apply_fin_img": True})
    both(f"img{ci} bwd_img declines", resblock, image=True, cin=ci, decline={"unetr_instnorm_bwd_img": True})
    case(f"img{ci} arena, no partial rows", resblock, image=True, cin=ci, arena=True, rows={"unetr_conv3_wgrad_rows": 0})
    case(f"img{ci} cout 8", resblock, image=True, cin=ci, cout=8)            # the fp32 image in front of the generic family
# -- each decline on its own
for kernel in ("unetr_conv3_fwd_parts", "unetr_instnorm_apply_fin", "unetr_conv3_dgrad_stats", "unetr_conv3_dgrad_fused", "unetr_instnorm_bwd_apply_fin"):
    case(f"res {kernel} declines", resblock, decline={kernel: True})
for n in (1, 2):
    case(f"res parts declines at call {n}", resblock, decline={"unetr_conv3_fwd_parts": {n}})
    case(f"res apply_fin declines at call {n}", resblock, decline={"unetr_instnorm_apply_fin": {n}})
case("res fused declines with w3", resblock, decline={"unetr_conv3_fwd_fused": {1}}, env={"UNETR_AMD_IN_FUSE": "2"})
case("res fused declines with and without w3", resblock, decline={"unetr_conv3_fwd_fused": {1, 2}}, env={"UNETR_AMD_IN_FUSE": "2"})
case("res fused declines", resblock, decline={"unetr_conv3_fwd_fused": True, "unetr_conv3_fwd_parts": True})
case("res fused declines, to_cat", resblock, to_cat=True, decline={"unetr_conv3_fwd_fused": True, "unetr_conv3_fwd_parts": True})
case("res wgrad_parts declines", resblock, arena=True, decline={"unetr_conv3_wgrad_parts": True})
case("res wgrad_parts declines at call 2", resblock, arena=True, decline={"unetr_conv3_wgrad_parts": {2}})
case("res cin 8, every fused kernel declines", resblock, cin=8, decline={k: True for k in (
    "unetr_conv3_fwd_parts", "unetr_conv3_fwd_fused", "unetr_conv3_dgrad_stats")})
# -- cout % 16 != 0: the generic im2col family
both("res cout 8", resblock, cout=8)
case("res cout 8, cin 8", resblock, cin=8, cout=8)
case("res cout 8 to_cat", resblock, cout=8, to_cat=True)
# -- transposed conv
both("tconv", tconv)
case("tconv to_cat", tconv, to_cat=True)
both("tconv no dx", tconv, need_dx=False)
case("tconv tokens", tconv, tokens=True)
case("tconv arena, no partial rows", tconv, arena=True, rows={"unetr_tconv2_wgrad_rows": 0})
for kernel in TCONV2_ARENA:
    case(f"tconv {kernel} declines", tconv, arena=kernel.endswith("parts"), decline={kernel: True})
case("tconv every dedicated kernel declines", tconv, decline={k: True for k in TCONV2})
case("tconv every dedicated kernel declines, to_cat, arena", tconv, to_cat=True, arena=True, decline={k: True for k in TCONV2_ARENA})
case("tconv tokens, every dedicated kernel declines", tconv, tokens=True, decline={k: True for k in TCONV2})
for co in (8, 6):                # the GEMM form: tap-major pack straight into a bf16 output; cout % 4 != 0: the pixel-shuffle tail
    both(f"tconv gemm cout {co}", tconv, precs=(1,), cin=64, cout=co)
    both(f"tconv gemm cout {co} no dx", tconv, precs=(1,), cin=64, cout=co, need_dx=False)
    case(f"tconv gemm cout {co} tokens", tconv, precs=(1,), cin=64, cout=co, tokens=True)
    case(f"tconv gemm cout {co} to_cat", tconv, precs=(1,), cin=64, cout=co, to_cat=True)
case("tconv cin 64, other modes", tconv, precs=(0, 2), cin=64, cout=8)
# -- the up block
for head in (False, True):
    h = " head" if head else ""
    both("up" + h, upblock, head=head)
    case(f"up{h} chain", upblock, head=head, skip="chain")
    case(f"up{h} IN_FUSE=0", upblock, head=head, env={"UNETR_AMD_IN_FUSE": "0"})
    case(f"up{h} OUT_FUSE=0", upblock, head=head, env={"UNETR_AMD_OUT_FUSE": "0"})
    case(f"up{h} parts declines", upblock, head=head, decline={"unetr_conv3_fwd_parts": True})
    case(f"up{h} stored route", upblock, head=head, arena=True, decline={k: True for k in (
        "unetr_conv3_fwd_parts", "unetr_conv3_fwd_fused", "unetr_conv3_dgrad_stats", "unetr_conv3_dgrad_fused", "unetr_conv3_wgrad_parts")})
    case(f"up{h} tconv2 declines", upblock, head=head, decline={k: True for k in TCONV2})
case("up fp32 skip", upblock, precs=(1,), skip="fp32")
case("up head chain arena", upblock, head=True, skip="chain", arena=True)
case("up no inp grad", upblock, inp_grad=False)
case("up refuses a plain skip", upblock, skip="refuse")
case("up gemm tconv", upblock, precs=(1,), cin=64, sp=(2, 2, 2))
case("up gemm tconv head arena", upblock, precs=(1,), cin=64, sp=(2, 2, 2), head=True, arena=True)
case("up head outconv_in_fwd declines", upblock, head=True, decline={"unetr_outconv_in_fwd": True})
case("up head outconv_in_fwd declines arena", upblock, head=True, arena=True, decline={"unetr_outconv_in_fwd": True})
case("up head bwd_apply_fin dual declines", upblock, head=True, decline={"unetr_instnorm_bwd_apply_fin": {1}})
case("up head bwd_apply_fin single declines", upblock, head=True, decline={"unetr_instnorm_bwd_apply_fin": {2}})
case("up head bwd_apply_fin declines", upblock, head=True, decline={"unetr_instnorm_bwd_apply_fin": True})
case("up head dgrad_stats declines", upblock, head=True, decline={"unetr_conv3_dgrad_stats": True})
case("up head dgrad_fused declines", upblock, head=True, decline={"unetr_conv3_dgrad_fused": True})
case("up head wgrad_parts declines", upblock, head=True, arena=True, decline={"unetr_conv3_wgrad_parts": True})
# -- the out conv, the public wrappers
both("outconv", outconv)
case("wrappers", wrappers)
case("wrappers, dedicated kernels decline", wrappers, decline={k: True for k in TCONV2_ARENA + (
    "unetr_conv3_fwd_parts", "unetr_conv3_fwd_fused", "unetr_instnorm_apply_fin", "unetr_instnorm_apply_fin_img", "unetr_instnorm_bwd_img",
    "unetr_instnorm_bwd_apply_fin", "unetr_conv3_dgrad_stats", "unetr_conv3_dgrad_fused", "unetr_outconv_in_fwd")})


def run_case(pkg, mp, name, cases=CASES, world_type=World):
    fn, prec, world, opt = cases[name]
    W = world_type(pkg, mp, prec, **world)
    try:
        fn(W, **opt)
    finally:
        W.close()
    return json.loads(json.dumps(W.log))


# the scenarios whose whole log is committed, entry by entry; every other scenario is committed as (number of entries, digest of them)
FULL = ("res cin 8, every fused kernel declines p1", "img1 arena p0", "tconv every dedicated kernel declines, to_cat, arena p1", "up head p1",
        "up head stored route p2")


def lines(log):
    return [json.dumps(e, separators=(",", ":")) for e in log]


def digest(log):
    return [len(log), hashlib.sha256("\n".join(lines(log)).encode()).hexdigest()[:16]]


@pytest.fixture(scope="module")
def parent_log():
    with open(LOG_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_match_the_parent_log(pkg, monkeypatch, parent_log, name):
    got = run_case(pkg, monkeypatch, name)
    for i, (g, w) in enumerate(zip(got, parent_log["full"].get(name, []))):
        assert g == w, f"{name}: entry {i} differs"
    # (a digest that differs: print both logs with the command in the module docstring and compare them)
    assert digest(got) == parent_log["digest"][name], f"{name}: not the parent's launches; this tree's are\n" + "\n".join(lines(got))
    # every kernel the scenario makes decline is launched in it: a decline that is never asked for pins nothing
    if not name.startswith("wrappers"):
        assert set(CASES[name][2].get("decline", {})) <= {e[0] for e in got}


def test_the_log_has_no_other_scenarios(parent_log):
    assert sorted(parent_log["digest"]) == sorted(CASES) and sorted(parent_log["full"]) == sorted(FULL)


def main(root, cases=CASES, full=FULL, run=run_case):
    sys.path.insert(0, os.path.abspath(root))
    pkg = importlib.import_module("3dmedicalimagesegmentation_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(root)
    logs = {}
    for name in cases:
        with pytest.MonkeyPatch.context() as mp:
            logs[name] = run(pkg, mp, name)
    if "--full" in sys.argv:          # every scenario entry by entry (to compare two trees)
        return print("\n".join(f"{name}: {line}" for name, log in logs.items() for line in lines(log)))
    dig = ",\n".join(f" {json.dumps(name)}: {json.dumps(digest(log))}" for name, log in logs.items())
    full = ",\n".join(f" {json.dumps(name)}: [\n" + ",\n".join(lines(logs[name])) + "\n ]" for name in full)
    print('{"digest": {\n' + dig + '\n},\n"full": {\n' + full + "\n}}")


if __name__ == "__main__":
    main(sys.argv[1])
