"""Host logic of the ViT side of functional.py on CPU tensors: which kernels TransformerBlockFn, PatchEmbedFn, LayerNormFn, TapFn and the
public ViT wrappers launch, in which order and with which arguments, on every route -- bf16 with the bf16 attention core (dh == 64) and
with fp32 attention on bf16 twins, the generic route that small or odd shapes fall to, fp32, bf16x3 with the LayerNorm riding on the GEMMs
and with each of its refusals -- crossed with the next block's norm, the tap twin, checkpointing, the prefetch neighbours and riders, the
transposed weight twins and arena mode.  The GPU tests reach the bf16 route at the benchmark's shape and little else of this.

The seams, `World` and the log format are those of tests/test_conv_routes_cpu.py; VitWorld adds the ViT side's environment switches,
PREFETCH_RIDERS, and in arena mode the arenas as UNETR.use_flat_buffers leaves them (a registered bf16 shadow arena and ArenaState.flat,
so that the word shadow and the transposed twins can exist; the twins are brought into being as tests/test_derived_weights_cpu.py does).
After each forward the log also says whether the result carries `_unetr_ln` (and where its three tensors live) and `_unetr_bf16`.
At the parent one pointer is logged as `other`, in the `noncontig` scenarios only: the contiguous copy of its input that
TransformerBlockFn.forward makes with Tensor.contiguous(), which no seam sees.

The expected logs (tests/vit_routes_parent_log.json) were NOT taken from the code under test: this driver was run against an untouched
checkout of commit df2c334 ("Conv-side blocks: one result record per route, pinned by a launch log"), the parent of the change that gave
the ViT blocks a route record and one activation record, and what it printed was committed: for every scenario the number of log entries
and a digest of them, and for a few representative scenarios (FULL) the whole log.  To print the same of any checkout:
python tests/test_vit_routes_cpu.py <checkout>   (with --full: every entry of every scenario, one per line, for a diff between two trees)."""
import contextlib
import json
import os
import sys
import types

import pytest
import torch

from test_conv_routes_cpu import World, digest, lines, main, run_case

ENV = ("UNETR_AMD_LN_RIDE", "UNETR_X3_GEMM_DMA", "UNETR_AMD_X3_WORDS", "UNETR_AMD_WT")
LOG_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vit_routes_parent_log.json")
F32, B16 = torch.float32, torch.bfloat16


class VitWorld(World):
    def __init__(self, pkg, mp, prec, env=None, arena=False, riders=True):
        self.riders = riders
        super().__init__(pkg, mp, prec, env=env, arena=arena)

    def install(self, env):
        super().install(env)
        for name in ENV:
            if name in env:
                self.mp.setenv(name, env[name])
            else:
                self.mp.delenv(name, raising=False)
        self.mp.setattr(self.Fn, "PREFETCH_RIDERS", self.riders)

    def weights(self, **shapes):
        """arena mode: the arenas as UNETR.use_flat_buffers leaves them -- parameters, gradients, and the registered bf16 shadow"""
        if not self.arena:
            return super().weights(**shapes)
        ga, dw = self.pkg.grad_arena, self.pkg.derived_weights
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in shapes.values()]
        offs, n = [], 0
        for p in ps:
            offs.append(n)
            n += (p.numel() + 7) // 8 * 8
        param, grad, shadow = self.know("param", torch.zeros(n)), self.know("grad", torch.zeros(n)), self.know("shadow", torch.zeros(n, dtype=B16))
        views = []
        for p, o in zip(ps, offs):
            p.data = param[o:o + p.numel()].view_as(p)
            views.append((p, grad[o:o + p.numel()].view_as(p)))
        self.st = ga.register_grad_sinks(views, ga.ArenaState())
        for p, o in zip(ps, offs):
            dw.register_weight_shadow(p, shadow[o:o + p.numel()].view_as(p))
        self.st.flat = dict(param=param, grad=grad, offsets=offs, params=ps, total=n, shadow=shadow, state=self.st)
        return ps

    def warm_twins(self, *ws):
        """current transposed twins of the Linear weights `ws`: asked for by a pass with the fused optimizer epilogue armed"""
        self.st.fuse = dict(index={})
        for w in ws:
            assert self.pkg.derived_weights.weight_bf16_t(w) is not None
        self.st.fuse = None
        self.know("twins", self.st.flat["shadow_t"])

    def warm_shadows(self, *ws):
        for w in ws:
            self.pkg.derived_weights.weight_bf16(w)

    def carries(self, t):
        ln, tw = getattr(t, "_unetr_ln", None), getattr(t, "_unetr_bf16", None)
        self.note("carries", {"ln": None if ln is None else [self.tensor(v) for v in ln[:3]], "bf16": None if tw is None else self.tensor(tw[0])})

    def forward(self, fn, *args):
        out = super().forward(fn, *args)
        self.carries(out)
        return out


# ------------------------------------------------------------------------------------------------------------------ scenarios
BLOCK = ("n1w", "n1b", "wqkv", "wp", "bp", "n2w", "n2b", "w1", "b1", "w2", "b2")          # TransformerBlockFn.apply's order


def block_shapes(hid, mlp, pre=""):
    shapes = dict(n1w=(hid,), n1b=(hid,), wqkv=(3 * hid, hid), wp=(hid, hid), bp=(hid,), n2w=(hid,), n2b=(hid,), w1=(mlp, hid), b1=(mlp,),
                  w2=(hid, mlp), b2=(hid,))
    return {pre + k: shapes[k] for k in BLOCK}


def block(W, M=8, hid=64, mlp=128, heads=1, next_ln=False, emit_twin=False, ckpt=False, no_grad=False, leaves=True, neighbours=None,
          twins=False, wt0=False):
    """one block; the neighbours' parameters (the next block's norm1 and qkv weight, linear2 / linear1 of the block below) live in the same
    arena.  neighbours: None, "cold" (no arena: they have no bf16 shadow yet) or "warm"; it implies the next block's norm, on whose ride the
    next qkv weight is prefetched"""
    B, L = 2, M // 2
    shapes = block_shapes(hid, mlp)
    shapes.update(nn1w=(hid,), nn1b=(hid,), nq=(3 * hid, hid), lw2=(hid, mlp), lw1=(mlp, hid))
    ps = dict(zip(shapes, W.weights(**shapes)))
    x = W.input("x", (M, hid), F32, grad=leaves)
    own = [ps[k] if leaves else ps[k].detach() for k in BLOCK]
    if neighbours == "warm" and not W.arena:
        W.warm_shadows(ps["nq"], ps["lw2"], ps["lw1"])
    if twins:
        W.warm_twins(*(ps[k] for k in ("wqkv", "wp", "w1", "w2")))
    if wt0:
        W.mp.setenv("UNETR_AMD_WT", "0")
    nxt = [ps[k].detach() if next_ln or neighbours else None for k in ("nn1w", "nn1b")]
    nb = [ps[k].detach() if neighbours else None for k in ("nq", "lw2", "lw1")]
    with torch.no_grad() if no_grad else contextlib.nullcontext():
        out = W.forward(W.Fn.TransformerBlockFn, x, *own, B, L, heads, W.prec, ckpt, *nxt, emit_twin, *nb)
    if no_grad or not leaves:
        return W.note("no backward", out.requires_grad)
    W.backward(out, x=x, **{k: ps[k] for k in BLOCK})


def chain(W, tap=False, cut=False, M=32, hid=64, mlp=128):
    """two blocks as UNETR._encode chains them: the second consumes the norm1 the first stashed, the first's backward the twin the
    second's attached; tap: the first is a tapped block (TapFn between them, the second consumer's gradient arrives on its own);
    cut: both aliases are parked on detached leaves, as UNETR._encode.cut does in staged mode"""
    Fn, B, L, b16 = W.Fn, 2, M // 2, W.prec == 1
    shapes = dict(block_shapes(hid, mlp, "a_"), **block_shapes(hid, mlp, "b_"))
    ps = dict(zip(shapes, W.weights(**shapes)))
    x = W.input("x", (M, hid), F32)
    stages = []

    def park(t):
        leaf = Fn.carry_twin(t, t.detach().requires_grad_(True))
        stages.append((t, leaf))
        return leaf
    xa = W.forward(Fn.TransformerBlockFn, x, *(ps["a_" + k] for k in BLOCK), B, L, 1, W.prec, False, ps["b_n1w"].detach(), ps["b_n1b"].detach(),
                   tap, ps["b_wqkv"].detach() if b16 else None, None, None)
    xb = None
    if tap:
        xa, xb = Fn.TapFn.apply(xa, b16)
        W.note("tap ->", W.tensor(xa), W.tensor(xb))
        for t in (xa, xb):
            W.carries(t)
        if cut:
            xb, xa = park(xb), park(xa)
    out = W.forward(Fn.TransformerBlockFn, xa, *(ps["b_" + k] for k in BLOCK), B, L, 1, W.prec, False, None, None, False, None,
                    ps["a_w2"].detach() if b16 else None, ps["a_w1"].detach() if b16 else None)
    dout = W.know("dout", torch.zeros(out.shape))
    dskip = W.know("dskip", torch.zeros(out.shape))
    W.note("backward")
    if cut:
        torch.autograd.backward([out], [dout])
        W.note("backward of the parked stage")
        (tb, lb), (ta, la) = stages
        torch.autograd.backward([ta, tb], [W.know("parked", la.grad), dskip])
    elif tap:
        torch.autograd.backward([out, xb], [dout, dskip])
    else:
        torch.autograd.backward([out], [dout])
    W.grads(x=x, **ps)


def noncontig(W, M=32, hid=64, mlp=128):
    """x is the left half of a wider buffer and carries a stashed norm1 and a bf16 twin: forward works on a contiguous copy"""
    Fn = W.Fn
    shapes = block_shapes(hid, mlp)
    ps = dict(zip(shapes, W.weights(**shapes)))
    base = W.input("base", (M, 2 * hid), F32)
    x = base[:, :hid]
    stash = [W.know("xn", torch.zeros(M, hid, dtype=B16 if W.prec == 1 else F32)), W.know("mean", torch.zeros(M)), W.know("rstd", torch.zeros(M))]
    Fn._stash_ln(x, ps["n1w"], ps["n1b"], *stash)
    Fn._attach_twin(x, W.know("xb", torch.zeros(M, hid, dtype=B16)))
    out = W.forward(Fn.TransformerBlockFn, x, *(ps[k] for k in BLOCK), 2, M // 2, 1, W.prec)
    W.backward(out, base=base, **ps)


def patch_embed(W, B=2):
    C, patch, hid, (D, H, Wd) = 1, 4, 64, (8, 8, 4)
    L = (D // patch) * (H // patch) * (Wd // patch)
    img = W.input("img", (B, C, D, H, Wd), F32, grad=False)
    w, b, pos = W.weights(w=(hid, C * patch ** 3), b=(hid,), pos=(1, L, hid))
    z = W.forward(W.Fn.PatchEmbedFn, img, w, b, pos, patch, W.prec)
    W.backward(z, w=w, b=b, pos=pos)


def layernorm(W, twin=False, below=False, M=8, hid=64, mlp=128):
    w, b, lw2, lw1 = W.weights(w=(hid,), b=(hid,), lw2=(hid, mlp), lw1=(mlp, hid))
    x = W.input("x", (M, hid), F32)
    if below and not W.arena:
        W.warm_shadows(lw2, lw1)
    y = W.forward(W.Fn.LayerNormFn, x, w, b, twin, lw2.detach() if below else None, lw1.detach() if below else None)
    W.backward(y, x=x, w=w, b=b)


def tap(W, want_bf16=True, one=False, M=8, hid=64):
    Fn = W.Fn
    g, b = W.weights(g=(hid,), b=(hid,))
    x = W.input("x", (M, hid), F32)
    Fn._stash_ln(x, g, b, W.know("xn", torch.zeros(M, hid, dtype=B16)), W.know("mean", torch.zeros(M)), W.know("rstd", torch.zeros(M)))
    Fn._attach_twin(x, W.know("xb", torch.zeros(M, hid, dtype=B16)))
    xa, xb = Fn.TapFn.apply(x, want_bf16)
    W.note("tap ->", W.tensor(xa), W.tensor(xb))
    for t in (xa, xb):
        W.carries(t)
    da, db = W.know("da", torch.zeros(M, hid)), W.know("db", torch.zeros(M, hid))
    W.note("backward")
    if one:          # (through autograd the missing gradient would arrive as zeros: the Function materialises them)
        ctx = types.SimpleNamespace(want_bf16=want_bf16)
        return W.note("one gradient ->", Fn.TapFn.backward(ctx, da, None)[0] is da, Fn.TapFn.backward(ctx, None, db)[0] is db)
    torch.autograd.backward([xa, xb], [da, db])
    W.grads(x=x)


def wrappers(W):
    """the public ViT wrappers that unetr.py, the tools and the GPU tests call directly, one step each"""
    Fn, prec = W.Fn, W.prec
    M, hid, mlp, B, L = 32, 64, 128, 2, 16

    def t(label, *shape, dtype=F32):
        return W.know(label, torch.zeros(*shape, dtype=dtype))

    def shown(r):
        if isinstance(r, (tuple, list)):
            return [shown(v) for v in r]
        if isinstance(r, W.capi.Prefetch):
            return W.plain(r)
        return W.tensor(r) if isinstance(r, torch.Tensor) else r

    def step(name, r):
        W.note(name + " ->", shown(r))
    w, bias, gam, bet, wq = W.weights(w=(mlp, hid), bias=(mlp,), gam=(hid,), bet=(hid,), wq=(hid, hid))
    x, res, pre, dy = t("x", M, hid), t("res", M, mlp), t("pre", M, mlp), t("dy", M, mlp)
    step("linear_fwd", Fn.linear_fwd(x, w, bias, prec, res=res, act=1, pre=pre))
    step("linear_fwd, periodic residual", Fn.linear_fwd(x, w, None, prec, res=t("pos", L, mlp), res_mod=L))
    step("linear_fwd, 8 rows", Fn.linear_fwd(x[:8], w, bias, prec))
    step("linear_dgrad", Fn.linear_dgrad(dy, w, prec))
    step("linear_dgrad through gelu'", Fn.linear_dgrad(dy, w, prec, aux=x))
    step("linear_wgrad", Fn.linear_wgrad(dy, x, prec))
    step("linear_wgrad, out", Fn.linear_wgrad(dy, x, prec, out=t("dw", mlp, hid)))
    step("colsum", Fn.colsum(dy, M, mlp, mlp))
    step("cast_bf16", Fn.cast_bf16(x))
    # gemm with the word shadow: a shape the Python gate takes (bf16x3 only), and one it refuses (8 rows)
    words = t("words", mlp, hid, dtype=torch.int32)
    step("gemm b_words", Fn.gemm(x, w, t("c", M, mlp), M, mlp, hid, lda=hid, ldb=hid, ldc=mlp, prec=prec, bias=bias, b_words=words))
    step("gemm b_words, 8 rows", Fn.gemm(x, w, t("c8", 8, mlp), 8, mlp, hid, lda=hid, ldb=hid, ldc=mlp, prec=prec, b_words=words))
    step("gemm b_words, b_trans", Fn.gemm(dy, w, t("cx", M, hid), M, hid, mlp, lda=mlp, ldb=hid, ldc=hid, prec=prec, b_trans=True, aux=x, ldaux=hid,
                                          act=2, accumulate=True, alpha=0.5, b_words=words))
    pf = Fn._prefetch("ln1_fwd", w, wq)
    step("_prefetch, no shadow yet", pf)
    W.warm_shadows(w)
    pf = Fn._prefetch("ln1_fwd", w, None, wq.detach())
    step("_prefetch", pf)
    step("_prefetch dgrad", Fn._prefetch("ln1_bwd", w.detach(), dgrad=M))
    xb = t("xb", M, hid, dtype=B16)
    y, mean, rstd = Fn.layernorm_fwd(x, gam, bet)
    step("layernorm_fwd", (y, mean, rstd))
    step("layernorm_fwd, bf16 only", Fn.layernorm_fwd(x, gam, bet, bf16_out=xb, want_fp32=False, pf=pf))
    dh_ = t("dh", M, hid)
    step("layernorm_bwd", Fn.layernorm_bwd(dh_, x, gam, mean, rstd))
    step("layernorm_bwd, everything", Fn.layernorm_bwd(dh_, x, gam, mean, rstd, dres=t("dres", M, hid), out_w=t("ow", hid), out_b=t("ob", hid),
                                                       dx_bf16=t("dxb", M, hid, dtype=B16), pf=pf))
    step("layernorm_bwd, part", Fn.layernorm_bwd(dh_, x, gam, mean, rstd, part=t("part", 8, 2 * hid)))
    step("layernorm_bwd_params", Fn.layernorm_bwd_params(dh_, x, gam, bet, mean, rstd, dres=t("dres2", M, hid), pf=pf))
    # the bf16-storage GEMM and the LayerNorm-riding forms
    ab, wb, wkn = t("ab", M, hid, dtype=B16), t("wb", mlp, hid, dtype=B16), t("wkn", hid, mlp, dtype=B16)
    step("gemm_bf16", Fn.gemm_bf16(ab, wb, M, mlp, hid, C=t("c2", M, mlp), bias=bias, res=res, ldr=mlp, act=1, pre=pre))
    step("gemm_bf16 b_kn, bf16 out", Fn.gemm_bf16(ab, wkn, M, mlp, hid, b_kn=True, Cb=t("cb", M, mlp, dtype=B16), act=2, aux=res, ldaux=mlp,
                                                  accumulate=True, alpha=2.0, ldcb=mlp, lda=hid, ldb=mlp, res_mod=L))
    dyb = t("dyb", M, mlp, dtype=B16)
    step("gemm_bf16_ln_fwd", Fn.gemm_bf16_ln_fwd(dyb, t("w2b", hid, mlp, dtype=B16), M, hid, mlp, t("c3", M, hid), gam, bet, xb, bias=bet, res=x,
                                                 ldr=hid, pf=pf))
    w2 = t("w2", hid, mlp)
    step("gemm_bf16_ln_fwd x3", Fn.gemm_bf16_ln_fwd(dy, w2, M, hid, mlp, t("c4", M, hid), gam, bet, None, y=t("y4", M, hid)))
    step("gemm_bf16_ln_fwd x3 words", Fn.gemm_bf16_ln_fwd(dy, w2, M, hid, mlp, t("c5", M, hid), gam, bet, None, y=t("y5", M, hid),
                                                          b_words=t("w2words", hid, mlp, dtype=torch.int32)))
    step("gemm_ln_bwd_params", Fn.gemm_ln_bwd_params(dyb, wb, M, hid, mlp, x, gam, bet, mean, rstd, dres=dh_, dx_bf16=t("dxb2", M, hid, dtype=B16), pf=pf))
    step("gemm_ln_bwd_params, twin", Fn.gemm_ln_bwd_params(dyb, wkn, M, hid, mlp, x, gam, bet, mean, rstd, b_kn=False))
    step("gemm_ln_bwd_params x3", Fn.gemm_ln_bwd_params(dy, w, M, hid, mlp, x, gam, bet, mean, rstd, dres=dh_))
    step("gemm_ln_bwd_params x3 words", Fn.gemm_ln_bwd_params(dy, w, M, hid, mlp, x, gam, bet, mean, rstd, b_words=words))
    # attention
    qkv, qkvb = t("qkv", M, 3 * hid), t("qkvb", M, 3 * hid, dtype=B16)
    att, lse = Fn.attention_fwd(qkv, B, L, 2, 32, prec, out_bf16=xb)
    step("attention_fwd", (att, lse))
    step("attention_bwd", Fn.attention_bwd(qkv, att, dh_, lse, B, L, 2, 32, prec, dqkv_bf16=t("dqkvb", M, 3 * hid, dtype=B16)))
    step("attention_bwd, no twin", Fn.attention_bwd(qkv, att, dh_, lse, B, L, 2, 32, prec))
    lse = Fn.attention_bf16_fwd(qkvb, B, L, 1, 64, xb, pf=pf)
    step("attention_bf16_fwd", lse)
    step("attention_bf16_fwd, fp32 out too", Fn.attention_bf16_fwd(qkvb, B, L, 1, 64, xb, out=t("att32", M, hid)))
    step("attention_bf16_bwd", Fn.attention_bf16_bwd(qkvb, xb, ab, lse, B, L, 1, 64, pf=pf))
    step("attention_bf16_bwd, fp32 out too", Fn.attention_bf16_bwd(qkvb, xb, ab, lse, B, L, 1, 64, dqkv=t("dqkv32", M, 3 * hid)))
    # twins
    s = Fn.add_cast(x, dh_)
    step("add_cast", (s, s._unetr_bf16[0]))
    s2 = Fn.add_cast(x, dh_, want_bf16=False)
    step("add_cast, no twin", (s2, hasattr(s2, "_unetr_bf16")))
    step("_twin, attached", Fn._twin(s))
    step("_twin, none attached", Fn._twin(s2))
    step("_twin of bf16", Fn._twin(xb))
    s.add_(1.0)
    step("_twin, stale", Fn._twin(s))
    Fn._stash_ln(s2, gam, bet, xb, mean, rstd)
    Fn._attach_twin(s2, xb)
    alias = Fn.carry_twin(s2, s2.view_as(s2))
    W.carries(alias)
    alias = Fn.carry_twin(s, s.view_as(s))
    W.carries(alias)
    step("gates", [Fn._bf16_path(prec, hid, mlp), Fn._bf16_path(prec, hid, 96), Fn.x3_ride_ok(M, hid, mlp), Fn.x3_ride_ok(8, hid, mlp),
                   Fn.x3_ride_ok(M, hid, 48), Fn.x3_ride_ok(M, 32, mlp), Fn.ln_ride_enabled()])


CASES = {}


def case(name, fn, precs=(0, 1, 2), reach=None, **opt):
    world = {k: opt.pop(k) for k in ("env", "arena", "riders") if k in opt}
    for prec in precs:
        CASES[f"{name} p{prec}"] = (fn, prec, world, opt, reach)


def both(name, fn, **opt):
    """a scenario with no arena and with its parameters in one"""
    case(name, fn, **opt)
    case(name + " arena", fn, arena=True, **opt)


# what a scenario is about must happen in it: predicates over the log's lines (one JSON list per entry, the kernel's name first)
def n(ls, *texts):
    return sum(all(t in line for t in texts) for line in ls)


def fwd(ls):
    return ls[:ls.index('["backward"]')] if '["backward"]' in ls else ls


def bwd(ls):
    return ls[ls.index('["backward"]'):]


def fast(ls, b16att=True):
    """the bf16 route: bf16 GEMMs, both LayerNorm backwards ride, the bf16 attention core or not"""
    return (n(fwd(ls), '["unetr_gemm_bf16"') >= 3 and n(bwd(ls), '["unetr_gemm_bf16_ln_bwd_pf"', '"x3":0') == 2 and not n(ls, '["unetr_gemm"')
            and bool(n(ls, '["unetr_attention_bf16_bwd_pf"')) == b16att and bool(n(ls, '["unetr_attention_bwd"')) != b16att)


def generic(ls):
    return not n(ls, '["unetr_gemm_bf16"') and not n(ls, '["unetr_gemm_bf16_ln') and n(fwd(ls), '["unetr_gemm"') == 4 and n(bwd(ls), '["unetr_layernorm_bwd_pf"') == 2


def x3ride(ls, words=None):
    """bf16x3 with both LayerNorm backwards riding on the data-gradient GEMMs (words: and reading the word shadow, or not)"""
    x3 = '"x3":' + ("" if words is None else "2" if words else "1")
    return n(bwd(ls), '["unetr_gemm_bf16_ln_bwd_pf"', x3) == 2 and not n(bwd(ls), '["unetr_layernorm_bwd_pf"')


def rides_fwd(ls):
    return n(fwd(ls), '["unetr_gemm_bf16_ln_fwd_pf"') == 1


ROUTES = {            # name -> (precision, options, the route's mark)
    "b16 dh64": (1, dict(), fast),
    "b16 dh32": (1, dict(heads=2), lambda ls: fast(ls, b16att=False)),
    "b16 M4": (1, dict(M=4), generic),
    "b16 mlp96": (1, dict(mlp=96), generic),
    "f32": (0, dict(), generic),
    "x3 M32": (2, dict(M=32), x3ride),
    "x3 M8": (2, dict(), generic),
    "x3 LN_RIDE=0": (2, dict(M=32, env={"UNETR_AMD_LN_RIDE": "0"}), generic),
    "x3 GEMM_DMA=0": (2, dict(M=32, env={"UNETR_X3_GEMM_DMA": "0"}), generic),
    "x3 X3_WORDS=0": (2, dict(M=32, env={"UNETR_AMD_X3_WORDS": "0"}), lambda ls: x3ride(ls, words=False)),
}
RIDES = ("b16 dh64", "b16 dh32", "x3 M32", "x3 X3_WORDS=0")          # the routes on which the next block's norm rides


def all_of(*preds):
    return lambda ls: all(p(ls) for p in preds)


for route, (prec, opt, mark) in ROUTES.items():
    one = dict(precs=(prec,), **opt)
    both(route, block, reach=mark, **one)
    rides = rides_fwd if route in RIDES else lambda ls: not rides_fwd(ls)
    both(route + " next_ln", block, next_ln=True, reach=all_of(mark, rides, lambda ls, r=route in RIDES: n(ls, '"ln":null') != r), **one)
    both(route + " emit_twin", block, emit_twin=True, reach=all_of(mark, lambda ls, f=route in RIDES[:2]: n(ls, '"bf16":null') != f), **one)
    # (the tapped block must not stash: its last GEMM writes the bf16 twin instead, on the bf16 routes)
    both(route + " next_ln emit_twin", block, next_ln=True, emit_twin=True, **one,
         reach=all_of(mark, lambda ls, x=route in RIDES[2:]: (not n(ls, '"ln":null')) == x and rides_fwd(ls) == x))
    both(route + " ckpt", block, ckpt=True, reach=mark, **one)
    both(route + " ckpt no_grad", block, ckpt=True, no_grad=True, **one)
    both(route + " ckpt no input grad", block, ckpt=True, leaves=False, **one)
case("x3 M32 words arena", block, precs=(2,), M=32, arena=True, next_ln=True, reach=lambda ls: x3ride(ls, words=True) and n(fwd(ls), '"x3":2') == 1)
case("f32 neighbours", block, precs=(0,), neighbours="warm", reach=lambda ls: not n(ls, '"ptr"'))
for route in ("b16 dh64", "b16 dh32"):
    prec, opt, mark = ROUTES[route]
    one = dict(precs=(prec,), **opt)
    both(route + " neighbours", block, neighbours="warm", **one,
         reach=all_of(mark, lambda ls: n(fwd(ls), '["unetr_gemm_bf16_ln_fwd_pf"', '"ptr":["') == 1 and n(bwd(ls), '"ptr":["', '",null]') < n(bwd(ls), '"ptr":["')))
    case(route + " neighbours cold", block, neighbours="cold", reach=lambda ls: n(fwd(ls), '["unetr_gemm_bf16_ln_fwd_pf"', '"ptr"') == 0, **one)
    both(route + " no riders", block, neighbours="warm", riders=False, reach=all_of(mark, lambda ls: not n(ls, '"ptr"')), **one)
    both(route + " riders ln1_fwd ln2_bwd", block, neighbours="warm", riders=("ln1_fwd", "ln2_bwd"), **one,
         reach=all_of(mark, lambda ls: n(ls, '["unetr_gemm_bf16_ln_fwd_pf"', '"ptr"') == 1 and n(ls, '["unetr_gemm_bf16_ln_bwd_pf"', '"ptr"') == 1
                      and not n(ls, '["unetr_attention', '"ptr"')))
    case(route + " twins arena", block, arena=True, twins=True, neighbours="warm", **one,
         reach=all_of(mark, lambda ls: n(bwd(ls), '"b_kn":0', '"twins+') == 4 and n(bwd(ls), '"ptr":["twins+') >= 1))
    case(route + " twins, UNETR_AMD_WT=0 arena", block, arena=True, twins=True, wt0=True, neighbours="warm", **one,
         reach=all_of(mark, lambda ls: not n(bwd(ls), '"twins+') and n(bwd(ls), '"b_kn":1') == 4))
case("b16 dh64 twins, M above WT_MAX_ROWS arena", block, precs=(1,), M=520, arena=True, twins=True, neighbours="warm",
     reach=all_of(fast, lambda ls: not n(bwd(ls), '"twins+') and n(bwd(ls), '"b_kn":1') == 4))
# -- two blocks chained; a non-contiguous input that carries a stash
both("chain", chain, reach=lambda ls: n(ls, '["unetr_layernorm_fwd_pf"') in (3, 4))            # (fp32: no ride, both norm1 launched)
both("chain tap", chain, tap=True, reach=lambda ls: n(ls, '["unetr_add_cast_bf16"') == 1)
both("chain tap cut", chain, tap=True, cut=True, reach=lambda ls: n(ls, '["unetr_add_cast_bf16"') == 1)
both("noncontig", noncontig, precs=(0,), reach=lambda ls: n(fwd(ls), '["unetr_layernorm_fwd_pf"') == 2)           # (fp32: no stash is read)
both("noncontig", noncontig, precs=(1, 2), reach=lambda ls: n(fwd(ls), '["unetr_layernorm_fwd_pf"') == 1)        # (the copy carries it)
# -- patch embedding, the final LayerNorm, the tap
both("patch", patch_embed, reach=lambda ls: n(ls, '["unetr_patch_gather"') == 1)
both("patch 4 rows", patch_embed, B=1, reach=lambda ls: not n(ls, '["unetr_gemm_bf16"'))
for twin in (False, True):
    for below in (False, True):
        both(f"layernorm twin={twin} below={below}", layernorm, precs=(1,), twin=twin, below=below,
             reach=lambda ls, pf=twin and below: n(ls, '"ptr"') == pf)
case("tap one gradient", tap, precs=(1,), one=True, reach=lambda ls: not n(ls, '["unetr_add_cast_bf16"'))
case("tap", tap, precs=(1,), reach=lambda ls: n(ls, '["unetr_add_cast_bf16"') == 1)
case("tap want_bf16=False", tap, precs=(1,), want_bf16=False, reach=lambda ls: n(ls, '["unetr_add_cast_bf16"', ",null,") == 1)
case("wrappers", wrappers)          # (outside a backward pass nothing can be deferred: no arena)

# the scenarios whose whole log is committed, entry by entry; every other scenario is committed as (number of entries, digest of them)
FULL = ("b16 dh64 neighbours arena p1", "x3 M32 next_ln arena p2", "patch p1")


def run(pkg, mp, name):
    return run_case(pkg, mp, name, cases={k: v[:4] for k, v in CASES.items()}, world_type=VitWorld)


@pytest.fixture(scope="module")
def parent_log():
    with open(LOG_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_match_the_parent_log(pkg, monkeypatch, parent_log, name):
    got = run(pkg, monkeypatch, name)
    for i, (g, w) in enumerate(zip(got, parent_log["full"].get(name, []))):
        assert g == w, f"{name}: entry {i} differs"
    # (a digest that differs: print both logs with the command in the module docstring and compare them)
    assert digest(got) == parent_log["digest"][name], f"{name}: not the parent's launches; this tree's are\n" + "\n".join(lines(got))
    # the switch, refusal or route the scenario names is reached in it, and no pointer is outside every labelled allocation
    reach = CASES[name][4]
    assert reach is None or reach(lines(got)), f"{name}: the scenario does not reach what it is about:\n" + "\n".join(lines(got))
    assert name.startswith("noncontig") or not n(lines(got), '"other"')


def test_the_log_has_no_other_scenarios(parent_log):
    assert sorted(parent_log["digest"]) == sorted(CASES) and sorted(parent_log["full"]) == sorted(FULL)


if __name__ == "__main__":
    main(sys.argv[1], cases=CASES, full=FULL, run=run)
