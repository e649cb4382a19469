"""Host logic of derived_weights.py on CPU tensors: the four kinds of derived weight copies are a state machine over version counters,
storage addresses, the weight epoch and the capture flag.  The ABI `call`, the stream lookup, the capture query and the pack-size query
are replaced (a recorder, a constant, a flag the test flips, a constant function); every step of a scenario asserts the exact list of
launches and the flags a caller can see.

The expected lists (EXPECTED, at the bottom) were NOT taken from derived_weights.py: the same scenarios were driven against
functional.py of the commit before the module existed, with the same seams patched there, and its log was written down here.
Pointers appear as byte offsets from the arena or buffer they point into."""
import ctypes
import gc
import types
import weakref

import pytest
import torch

STREAM = 77
F32, BF16 = 0, 1          # _capi.PREC_F32, _capi.PREC_BF16


class DeviceParameter(torch.nn.Parameter):
    """a CPU parameter that claims a device: refresh_conv_packs leaves CPU parameters alone"""
    is_cuda = True


class Model:
    def __init__(self, params, flat):
        self._params, self._flat = list(params), flat

    def parameters(self):
        return iter(self._params)


class World:
    """Six CPU parameters in hand-built flat arenas registered with one ArenaState, as UNETR.use_flat_buffers leaves them (every bf16
    shadow slice registered as optimizer-maintained), and a parameter `lone` outside any arena.  `step` closes one step of a scenario:
    the launches since the last one and the flags the test read, checked against the parent's log."""
    SHAPES = [(8, 16), (16, 8), (5,), (12, 8), (4, 2, 3, 3, 3), (8,)]      # 2 twin-able Linear weights, a padded bias, N % 8 != 0, a conv weight

    def __init__(self, pkg, monkeypatch):
        self.pkg, self.mp = pkg, monkeypatch
        self.capturing = False
        self.launches, self.events, self.expect, self.known = [], [], None, []
        self.install()
        self.params = [(DeviceParameter if len(s) == 5 else torch.nn.Parameter)(torch.zeros(s)) for s in self.SHAPES]
        self.offs, n = [], 0
        for p in self.params:
            self.offs.append(n)
            n += (p.numel() + 7) // 8 * 8
        arena, grad, shadow = torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=torch.bfloat16)
        views = []
        for p, o in zip(self.params, self.offs):
            p.data = arena[o:o + p.numel()].view_as(p)
            views.append((p, grad[o:o + p.numel()].view_as(p)))
        self.st = pkg.grad_arena.register_grad_sinks(views, pkg.grad_arena.ArenaState())
        for p, o in zip(self.params, self.offs):
            self.dw.register_weight_shadow(p, shadow[o:o + p.numel()].view_as(p))
        self.flat = dict(param=arena, grad=grad, offsets=self.offs, params=self.params, total=n, shadow=shadow, state=self.st)
        self.st.flat = self.flat
        self.know("param", arena)
        self.know("shadow", shadow)
        self.lone = torch.nn.Parameter(torch.zeros(8, 8))
        self.know("lone", self.lone)
        self.model = Model(self.params + [self.lone], self.flat)

    # ---- the seams (a driver for another commit overrides these) ----
    def install(self):
        self.dw = dw = self.pkg.derived_weights
        self.mp.setattr(dw, "call", self.record)
        self.mp.setattr(dw, "_stream", lambda: STREAM)
        self.mp.setattr(dw, "_capturing", lambda: self.capturing)
        self.mp.setattr(dw, "_pack_bytes", lambda w, kind, prec: 64 + 16 * kind + 8 * prec)
        for kind in (dw.BF16, dw.WORDS, dw.TWIN, dw.PACK):      # empty tables: refresh_conv_packs takes every live conv weight of the process
            self.mp.setattr(kind, "table", {})
            self.mp.setattr(kind, "by_addr", {})
        self.mp.setattr(self.pkg.functional, "workspace", lambda device: self.flat["grad"])      # (SlidingWindowInferer._signature)

    def maintained(self, w, *pack):
        return next(r.maintained for r in self.dw.records_of([w]) if r.kind.name != "x3" and r.pack == pack)

    def trailer(self, form, stepped, wt_done=()):
        """the call optim.AdamW makes at the end of each of its stepping forms"""
        if form == "per_tensor":
            self.dw.after_step(self.flat, stepped, arena=False)
        elif form == "flat":
            self.dw.after_step(self.flat, stepped, arena=True, repack=False)
        elif form == "fused_finish":
            self.dw.after_step(self.flat, stepped, arena=True, twins_written=wt_done)
        else:
            assert form == "reduced_end"
            self.dw.after_step(self.flat, stepped, arena=True)

    def describe(self, rec):
        return (rec.kind.name, self.where(rec.param().data_ptr())) + tuple(rec.pack)

    def captured_row(self):
        """what SlidingWindowInferer._capture keeps of a captured forward"""
        swi = self.pkg.inference.SlidingWindowInferer
        derived = swi._derived_entries(self.model)
        return types.SimpleNamespace(as_is=swi._as_is(self.model), derived=derived, static_in=self.flat["grad"],
                                     signature=swi._signature(self.model, None, derived))

    # ---- recorder ----
    def know(self, label, t):
        self.known.append((label, t))          # (keeps the tensor alive: its address is never reused)
        return t

    def where(self, v):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if v is None or isinstance(v, (bool, float)) or not isinstance(v, int):
            return v
        for label, t in self.known:
            if t.data_ptr() <= v < t.data_ptr() + max(1, t.numel()) * t.element_size():
                return f"{label}+{v - t.data_ptr()}"
        return v

    def record(self, name, *args):
        self.launches.append((name, args))

    def _snap(self, a):
        if isinstance(a, ctypes.Array):
            if issubclass(a._type_, ctypes.Structure):
                return [{f: self.where(getattr(e, f)) for f, _ in e._fields_} for e in a]
            return [self.where(x) for x in a]
        return self.where(a)

    def step(self, label, **flags):
        # (structs are snapshot when the step closes: the buffers a getter has just created are known by then; nothing rewrites them)
        got = (label, [(name,) + tuple(self._snap(a) for a in args) for name, args in self.launches], flags)
        self.launches = []
        self.events.append(got)
        if self.expect is not None:
            assert len(self.events) <= len(self.expect), f"step {label!r} is not in the parent's log"
            assert got == self.expect[len(self.events) - 1]

    def bump(self, *ps):
        with torch.no_grad():
            for p in ps:
                p.add_(1.0)           # torch modifies the parameter: the version counter moves

    def prefetch(self, *ws, dgrad=0):
        pf = self.pkg.functional._prefetch("ln1_bwd" if dgrad else "ln1_fwd", *ws, dgrad=dgrad)
        return None if pf is None else [(self.where(pf.ptr[i]), pf.bytes[i]) for i in range(2) if pf.ptr[i]]


# -------------------------------------------------------------------------------------------------------------- scenarios
def scenario_bf16(W):
    dw, w, st, p = W.dw, W.lone, W.st, W.params
    sh = W.know("sh_lone", dw.weight_bf16(w))
    W.step("first get derives", maintained=W.maintained(w), shape=tuple(sh.shape), dtype=str(sh.dtype))
    assert dw.weight_bf16(w) is sh
    W.step("second get in the same epoch does not")
    dw.begin_forward()
    assert dw.weight_bf16(w) is sh
    W.step("a new epoch re-derives an unmaintained copy")
    W.step("the optimizer takes the pointer", ptr=W.where(dw.shadow_ptr_for_update(w)), maintained=W.maintained(w))
    dw.begin_forward()
    dw.weight_bf16(w)
    W.step("a new epoch keeps a maintained copy")
    W.bump(w)
    W.step("no pointer for an out-of-step copy", ptr=W.where(dw.shadow_ptr_for_update(w)), maintained=W.maintained(w))
    dw.weight_bf16(w)
    W.step("version bump re-derives", maintained=W.maintained(w))
    dw.shadow_ptr_for_update(w)
    w.data = W.know("lone2", torch.zeros(8, 8))
    W.step("re-pointed .data: no pointer", ptr=W.where(dw.shadow_ptr_for_update(w)))
    assert dw.weight_bf16(w) is sh
    W.step("re-pointed .data re-derives", maintained=W.maintained(w))
    dw.shadow_ptr_for_update(w)
    dw.invalidate_weight_shadows()
    W.step("invalidate: no pointer", ptr=W.where(dw.shadow_ptr_for_update(w)))
    dw.weight_bf16(w)
    W.step("invalidate re-derives", maintained=W.maintained(w))
    dw.weight_bf16(w)
    W.step("same epoch again: nothing")
    W.capturing = True
    dw.begin_forward()                    # (a forward being captured does not start an epoch)
    dw.weight_bf16(w)
    dw.weight_bf16(w)
    W.step("under capture an unmaintained copy always re-derives")
    W.capturing = False
    dw.weight_bf16(w)
    W.step("capture did not start an epoch")
    W.capturing = True
    dw.shadow_ptr_for_update(w)
    dw.weight_bf16(w)
    W.step("under capture a maintained copy never does")
    W.capturing = False
    w.data = W.know("lone3", torch.zeros(4, 8))
    sh2 = W.know("sh_lone3", dw.weight_bf16(w))
    W.step("another shape: another buffer", shape=tuple(sh2.shape), same=sh2 is sh)


def scenario_arena_bf16(W):
    """the arena shadows (registered by use_flat_buffers as maintained) and mark_flat_maintained"""
    dw, st, p = W.dw, W.st, W.params
    W.know("sh_lone", dw.weight_bf16(W.lone))
    W.step("a registered shadow is the arena slice", buf=W.where(dw.weight_bf16(p[1]).data_ptr()), unmaintained=st.unmaintained)
    W.bump(p[0], p[1])
    dw.mark_flat_maintained(p[:2], st)
    W.step("mark_flat_maintained returns early while nothing was re-derived", ptr=W.where(dw.shadow_ptr_for_update(p[0])),
           unmaintained=st.unmaintained)
    dw.weight_bf16(p[0])
    W.step("a re-derived arena shadow is counted", maintained=W.maintained(p[0]), unmaintained=st.unmaintained)
    dw.mark_flat_maintained(p[:2], st)
    W.step("mark_flat_maintained walks and zeroes the count", maintained=W.maintained(p[0]), unmaintained=st.unmaintained,
           ptr0=W.where(dw.shadow_ptr_for_update(p[0])), ptr1=W.where(dw.shadow_ptr_for_update(p[1])))
    W.bump(p[1])
    dw.weight_bf16(p[1])
    dw.mark_flat_maintained(p[:2])                    # (the state is looked up from the first parameter)
    W.step("mark_flat_maintained finds the owner itself", maintained=W.maintained(p[1]), unmaintained=st.unmaintained)
    p[0].data = W.know("moved", torch.zeros(8, 16))
    st.unmaintained = 1
    dw.mark_flat_maintained(p[:2], st)
    W.step("a moved parameter is not vouched for", ptr=W.where(dw.shadow_ptr_for_update(p[0])), unmaintained=st.unmaintained)
    W.step("prefetch names existing shadows by address", pf=W.prefetch(p[1].detach(), W.lone.detach()), moved=W.prefetch(p[0].detach()), none=W.prefetch(torch.zeros(3)))


def scenario_packs(W):
    dw, cw = W.dw, W.params[4]
    bufs = {}
    for kind, prec in [(0, F32), (1, F32), (0, BF16)]:
        bufs[kind, prec] = W.know(f"pack{kind}{prec}", dw.conv_pack_get(cw, kind, prec))
    W.step("first get packs each (kind, precision)", sizes=[b.numel() for b in bufs.values()], maintained=W.maintained(cw, 0, F32))
    for key, b in bufs.items():
        assert dw.conv_pack_get(cw, *key) is b
    W.step("second get in the same epoch does not")
    dw.begin_forward()
    dw.conv_pack_get(cw, 1, F32)
    W.step("a new epoch re-packs an unmaintained pack")
    cpu = torch.nn.Parameter(torch.zeros(4, 2, 3, 3, 3))
    W.know("cpu", cpu)
    W.know("pack_cpu", dw.conv_pack_get(cpu, 0, F32))
    dying = DeviceParameter(torch.zeros(2, 2, 3, 3, 3))
    W.know("dying", dying.data)
    ref = weakref.ref(dw.conv_pack_get(dying, 0, F32))
    W.know("pack_dying", ref())
    W.step("two more weights")
    W.known.pop()                         # from here on only the record holds the dying weight's pack: pruning it frees the buffer
    del dying
    gc.collect()
    held = ref() is not None
    W.bump(cw)
    dw.refresh_conv_packs()
    W.step("refresh skips what torch touched and prunes the dead", held_before=held, pruned=ref() is None,
           maintained=W.maintained(cw, 0, F32), cpu=W.maintained(cpu, 0, F32))
    for key in bufs:
        dw.conv_pack_get(cw, *key)
    dw.refresh_conv_packs()
    W.step("refresh: one launch per precision", maintained=[W.maintained(cw, *k) for k in bufs], cpu=W.maintained(cpu, 0, F32))
    dw.begin_forward()
    for key in bufs:
        dw.conv_pack_get(cw, *key)
    W.step("a new epoch keeps maintained packs")
    W.bump(cw)
    dw.conv_pack_get(cw, 0, BF16)
    W.step("version bump re-packs", maintained=[W.maintained(cw, *k) for k in bufs])
    dw.refresh_conv_packs()
    W.step("refresh takes only the packs in step", maintained=[W.maintained(cw, *k) for k in bufs])
    W.capturing = True
    dw.conv_pack_get(cw, 0, BF16)
    dw.conv_pack_get(cpu, 0, F32)
    dw.conv_pack_get(cpu, 0, F32)
    W.step("under capture: maintained never, unmaintained always")
    W.capturing = False
    dw.invalidate_weight_shadows()
    dw.refresh_conv_packs()
    W.step("invalidate: refresh finds nothing in step")
    dw.conv_pack_get(cw, 0, BF16)
    W.step("invalidate re-packs", maintained=W.maintained(cw, 0, BF16))
    cw.data = W.know("cw2", torch.zeros(4, 2, 3, 3, 3))
    assert dw.conv_pack_get(cw, 0, BF16) is bufs[0, BF16]
    W.step("re-pointed .data re-packs")


def scenario_words(W):
    dw, p, flat = W.dw, W.params, W.flat
    dw.refresh_x3_shadow(flat)
    W.capturing = True
    W.step("absent under capture: None, and no arena", got=dw.weight_x3(p[0]), arena=flat.get("shadow_x3") is not None)
    W.capturing = False
    ws = dw.weight_x3(p[0])
    W.know("words", flat["shadow_x3"])
    W.step("first use: one launch over the whole arena", buf=W.where(ws.data_ptr()), shape=tuple(ws.shape), dtype=str(ws.dtype))
    W.step("every parameter of the arena has its slice", bias=W.where(dw.weight_x3(p[2]).data_ptr()), lone=dw.weight_x3(W.lone))
    W.bump(p[2])
    dw.begin_forward()
    dw.weight_x3(p[0])
    dw.weight_x3(p[2])
    W.step("version bump re-splits the padded slot; the epoch does not matter")
    W.bump(p[0])
    W.capturing = True
    dw.weight_x3(p[0])
    dw.weight_x3(p[0])
    W.step("a stale slice under capture")
    W.capturing = False
    W.bump(p[0], p[1])
    dw.refresh_x3_shadow(flat)
    dw.weight_x3(p[0])
    dw.weight_x3(p[1])
    W.step("refresh, not written: one derive launch, every slice stamped")
    W.bump(p[0])
    dw.refresh_x3_shadow(flat, written=True)
    dw.weight_x3(p[0])
    W.step("refresh, written: stamped without a launch")
    dw.invalidate_weight_shadows()
    dw.weight_x3(p[1])
    W.step("invalidate re-splits")
    W.mp.setenv("UNETR_AMD_X3_WORDS", "0")
    W.step("UNETR_AMD_X3_WORDS=0", got=dw.weight_x3(p[1]))
    W.mp.delenv("UNETR_AMD_X3_WORDS")
    p[1].data = W.know("moved", torch.zeros(16, 8))
    dw.refresh_x3_shadow(flat, written=True)
    W.step("a moved parameter has no words", got=dw.weight_x3(p[1]), other=W.where(dw.weight_x3(p[0]).data_ptr()))


def scenario_twins(W):
    dw, p, flat, st = W.dw, W.params, W.flat, W.st
    W.step("no armed epilogue: no twin, no arena", got=dw.weight_bf16_t(p[0]), arena="shadow_t" in flat)
    st.fuse = dict(kind="bf16out")
    W.step("the bf16 communication epilogue does not count", got=dw.weight_bf16_t(p[0]), arena="shadow_t" in flat)
    st.fuse = dict(index={})
    W.capturing = True
    W.step("never created under capture", got=dw.weight_bf16_t(p[0]), arena="shadow_t" in flat)
    W.capturing = False
    t0 = dw.weight_bf16_t(p[0])
    W.know("twins", flat["shadow_t"])
    W.step("armed AdamW epilogue: the arena is created, zero-filled, and the twin derived", buf=W.where(t0.data_ptr()),
           shape=tuple(t0.shape), dtype=str(t0.dtype), zero=not bool(flat["shadow_t"].count_nonzero()), epilogue=dw._epilogue_twin_arena(flat) is flat["shadow_t"])
    t1 = dw.weight_bf16_t(p[1])
    W.step("the second weight", buf=W.where(t1.data_ptr()), shape=tuple(t1.shape))
    W.step("no twin for 1-D, unaligned, conv or foreign weights", got=[dw.weight_bf16_t(w) for w in (p[2], p[3], p[4], W.lone)])
    assert dw.weight_bf16_t(p[0]) is t0 and dw.weight_bf16_t(p[1]) is t1
    W.step("current twins are handed out")
    W.step("prefetch names the twin of a data-gradient GEMM", pf=W.prefetch(p[0].detach(), p[3].detach(), dgrad=16),
           big=W.prefetch(p[0].detach(), dgrad=4096), fwd=W.prefetch(p[0].detach()))
    st.fuse = None
    W.step("an existing arena serves a pass without epilogue", same=dw.weight_bf16_t(p[0]) is t0)
    W.capturing = True
    W.step("under capture without epilogue: None", got=dw.weight_bf16_t(p[0]), pf=W.prefetch(p[0].detach(), dgrad=16))
    st.fuse = dict(index={})
    W.step("under capture with it: the current twin", same=dw.weight_bf16_t(p[0]) is t0, pf=W.prefetch(p[0].detach(), dgrad=16))
    W.bump(p[0])
    W.step("under capture a stale twin is not handed out", got=dw.weight_bf16_t(p[0]), pf=W.prefetch(p[0].detach(), dgrad=16))
    W.capturing = False
    W.bump(p[1])
    assert dw.weight_bf16_t(p[1]) is t1
    W.step("every stale twin of the arena in one grouped launch", unmaintained=st.unmaintained)
    dw.invalidate_weight_shadows()
    assert dw.weight_bf16_t(p[0]) is t0
    W.step("after invalidate: all of them")
    dw.mark_flat_maintained(p[:2], st)
    dw.refresh_wt_shadow(flat, p[:4], written=[p[1]])
    W.step("refresh: a written twin keeps its stamp, the others are re-derived")
    W.bump(p[1])
    dw.weight_bf16(p[1])
    dw.mark_flat_maintained(p[:2], st)
    dw.refresh_wt_shadow(flat, p[:2], written=[p[1]])
    W.step("written and stale stays stale", pf=W.prefetch(p[1].detach(), dgrad=16))
    dw.weight_bf16_t(p[1])
    W.step("the next pass re-derives it")
    W.capturing = True
    dw.refresh_wt_shadow(flat, p[:1])
    W.capturing = False
    W.step("a captured step only marks stale", pf=W.prefetch(p[0].detach(), dgrad=16))
    dw.weight_bf16_t(p[0])
    W.step("and the next eager pass re-derives")
    W.bump(p[0])
    dw.refresh_wt_shadow(flat, p[:2])
    W.step("refresh with an out-of-step shadow marks stale, derives the rest")
    W.mp.setenv("UNETR_AMD_WT", "0")
    W.step("UNETR_AMD_WT=0", got=dw.weight_bf16_t(p[1]), epilogue=dw._epilogue_twin_arena(flat), pf=W.prefetch(p[1].detach(), dgrad=16))
    W.mp.delenv("UNETR_AMD_WT")
    st.clear()                            # (ArenaState.clear -> drop_wt_shadow; the sinks are gone with it)
    W.step("ArenaState.clear drops the arena and its entries", arena="shadow_t" in flat, pf=W.prefetch(p[1].detach(), dgrad=16))
    dw.drop_wt_shadow(flat)
    dw.drop_wt_shadow(None)
    views = [(q, flat["grad"][o:o + q.numel()].view_as(q)) for q, o in zip(p, W.offs)]
    W.pkg.grad_arena.register_grad_sinks(views, st)
    st.fuse = dict(index={})
    t = dw.weight_bf16_t(p[1])
    W.know("twins2", flat["shadow_t"])
    W.step("a new arena after the drop", buf=W.where(t.data_ptr()), same=t is t1)
    st.fuse = None


def _warm(W):
    """every kind exists: words, twins of p0 / p1, two packs of the conv weight"""
    dw, p, flat, st = W.dw, W.params, W.flat, W.st
    dw.weight_x3(p[0])
    W.know("words", flat["shadow_x3"])
    st.fuse = dict(index={})
    dw.weight_bf16_t(p[0])
    dw.weight_bf16_t(p[1])
    st.fuse = None
    W.know("twins", flat["shadow_t"])
    W.know("pack00", dw.conv_pack_get(p[4], 0, F32))
    W.know("pack01", dw.conv_pack_get(p[4], 0, BF16))
    W.step("warm")


def scenario_trailers(W):
    dw, p, st = W.dw, W.params, W.st
    _warm(W)
    stepped = p[:5]                      # (p[5] received no gradient)

    def flags():
        return dict(unmaintained=st.unmaintained, packs=[W.maintained(p[4], 0, F32), W.maintained(p[4], 0, BF16)],
                    bf16=[W.maintained(q) for q in p[:2]], twins=W.prefetch(p[0].detach(), p[1].detach(), dgrad=16))
    for q in stepped:                    # the per-tensor kernels take each shadow's pointer
        dw.shadow_ptr_for_update(q)
    W.trailer("per_tensor", stepped)
    W.step("per-tensor step", **flags())
    W.trailer("flat", stepped)
    W.step("flat step", **flags())
    W.trailer("fused_finish", stepped, wt_done=[p[1]])
    W.step("fused finish", **flags())
    W.trailer("reduced_end", stepped)
    W.step("reduced end", **flags())
    # torch touched two weights, and one of them was read since: the arena kernels' step vouches for both again
    W.bump(p[0], p[1])
    dw.begin_forward()
    dw.weight_bf16(p[0])
    dw.conv_pack_get(p[4], 0, F32)
    W.step("between steps", **flags())
    W.trailer("flat", stepped)
    W.step("flat step after torch touched weights", **flags())
    W.bump(p[0], p[4])
    dw.weight_bf16(p[0])
    W.trailer("fused_finish", stepped, wt_done=[p[0]])
    W.step("fused finish after torch touched weights", **flags())
    dw.weight_x3(p[0])
    dw.weight_bf16_t(p[0])
    dw.conv_pack_get(p[4], 0, F32)
    W.step("what the next pass re-derives")
    W.bump(p[1])
    W.capturing = True
    W.trailer("reduced_end", stepped)
    W.capturing = False
    W.step("reduced end under capture", **flags())


def scenario_listing(W):
    dw, p, lone = W.dw, W.params, W.lone
    swi = W.pkg.inference.SlidingWindowInferer
    _warm(W)

    def as_is():
        return [W.describe(r) for r in swi._as_is(W.model)]
    W.know("sh_lone", dw.weight_bf16(lone))
    W.step("before a step: maintained arena shadows and the words; neither the cast shadow nor the packs", as_is=as_is(),
           listed=[W.describe(r) for r in swi._derived_entries(W.model)])
    W.trailer("flat", p[:5])
    dw.refresh_conv_packs()
    dw.shadow_ptr_for_update(lone)
    W.step("after a step: everything", as_is=as_is())
    row = W.captured_row()
    W.bump(p[0])
    W.step("torch touched a weight: its shadow and words drop out", as_is=as_is())
    W.step("refresh re-derives what the graph reads as it is; nothing moved", ok=swi._refresh(swi, W.model, [row, row]),
           same=row.signature == swi._signature(W.model, None, row.derived))
    W.step("the next call starts an epoch: the copy that is no longer maintained is re-derived again", ok=swi._refresh(swi, W.model, [row]))
    dw.invalidate_weight_shadows()
    W.step("after invalidate: every as-is copy", ok=swi._refresh(swi, W.model, [row]), as_is=as_is())
    lone.data = W.know("lone2", torch.zeros(8, 8))
    W.step("a parameter moved: capture again", ok=swi._refresh(swi, W.model, [row]))
    row = W.captured_row()
    W.step("the new capture is stable", ok=swi._refresh(swi, W.model, [row]), as_is=as_is())
    lone.data = W.know("lone3", torch.zeros(8, 8))
    row.signature = swi._signature(W.model, None, row.derived)
    lone.data = W.know("lone4", torch.zeros(4, 8))
    W.know("sh_lone4", dw.weight_bf16(lone))                   # (another shape: the getter registers another buffer)
    sig = swi._signature(W.model, None, row.derived)
    W.step("a derived buffer moved: the signature differs there only",
           diff=[i for i, (a, b) in enumerate(zip(row.signature, sig)) if a != b], n=len(sig))
    W.capturing = True
    with pytest.raises(RuntimeError, match="captured"):
        dw.refresh_derived_weights(W.model)
    W.capturing = False
    W.bump(p[0], p[1], p[4])
    dw.refresh_derived_weights(W.model)
    W.step("refresh_derived_weights: bf16, words, packs, then the twins")
    dw.refresh_derived_weights(W.model)
    W.step("and nothing when all is current")


SCENARIOS = dict(bf16=scenario_bf16, arena_bf16=scenario_arena_bf16, packs=scenario_packs, words=scenario_words, twins=scenario_twins, trailers=scenario_trailers,
                 listing=scenario_listing)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario_matches_the_parent_log(pkg, monkeypatch, name):
    W = World(pkg, monkeypatch)
    W.expect = EXPECTED[name]
    try:
        SCENARIOS[name](W)
    finally:
        W.st.fuse = None
        pkg.grad_arena.clear_grad_sinks(W.st)
    assert len(W.events) == len(W.expect)


def test_module_seams(pkg):
    """derived_weights stands below functional (which only re-exports it), and grad_arena's twin hooks come from it"""
    dw, Fn, ga = pkg.derived_weights, pkg.functional, pkg.grad_arena
    assert "functional" not in vars(dw) and ga._drop_twins is dw.drop_wt_shadow and ga._twin_arena is dw._epilogue_twin_arena
    for name in ("weight_bf16", "weight_x3", "weight_bf16_t", "conv_pack_get", "register_weight_shadow", "shadow_ptr_for_update",
                 "drop_wt_shadow", "invalidate_weight_shadows", "refresh_derived_weights"):
        assert getattr(Fn, name) is getattr(dw, name)
    assert pkg.invalidate_weight_shadows is dw.invalidate_weight_shadows and pkg.refresh_derived_weights is dw.refresh_derived_weights


# the parent's log, as its driver printed it
EXPECTED = {'bf16': [('first get derives', [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)], {'maintained': False, 'shape': (8, 8), 'dtype': 'torch.bfloat16'}),
          ('second get in the same epoch does not', [], {}),
          ('a new epoch re-derives an unmaintained copy', [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)], {}),
          ('the optimizer takes the pointer', [], {'ptr': 'sh_lone+0', 'maintained': True}),
          ('a new epoch keeps a maintained copy', [], {}),
          ('no pointer for an out-of-step copy', [], {'ptr': None, 'maintained': True}),
          ('version bump re-derives', [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)], {'maintained': False}),
          ('re-pointed .data: no pointer', [], {'ptr': None}),
          ('re-pointed .data re-derives', [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)], {'maintained': False}),
          ('invalidate: no pointer', [], {'ptr': None}),
          ('invalidate re-derives', [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)], {'maintained': False}),
          ('same epoch again: nothing', [], {}),
          ('under capture an unmaintained copy always re-derives',
           [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77), ('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)],
           {}),
          ('capture did not start an epoch', [], {}),
          ('under capture a maintained copy never does', [], {}),
          ('another shape: another buffer', [('unetr_cast_bf16', 'lone+0', 'sh_lone3+0', 32, 77)], {'shape': (4, 8), 'same': False})],
 'arena_bf16': [('a registered shadow is the arena slice', [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)], {'buf': 'shadow+256', 'unmaintained': 0}),
                ('mark_flat_maintained returns early while nothing was re-derived', [], {'ptr': None, 'unmaintained': 0}),
                ('a re-derived arena shadow is counted', [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77)], {'maintained': False, 'unmaintained': 1}),
                ('mark_flat_maintained walks and zeroes the count', [], {'maintained': True, 'unmaintained': 0, 'ptr0': 'shadow+0', 'ptr1': 'shadow+256'}),
                ('mark_flat_maintained finds the owner itself',
                 [('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77)],
                 {'maintained': True, 'unmaintained': 0}),
                ('a moved parameter is not vouched for', [], {'ptr': None, 'unmaintained': 0}),
                ('prefetch names existing shadows by address', [], {'pf': [('shadow+256', 256), ('sh_lone+0', 128)], 'moved': None, 'none': None})],
 'packs': [('first get packs each (kind, precision)',
            [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
             ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack10+0', 'Cin': 2, 'Cout': 4, 'kind': 1}], 1, 0, 77),
             ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
            {'sizes': [64, 80, 72], 'maintained': False}),
           ('second get in the same epoch does not', [], {}),
           ('a new epoch re-packs an unmaintained pack',
            [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack10+0', 'Cin': 2, 'Cout': 4, 'kind': 1}], 1, 0, 77)],
            {}),
           ('two more weights',
            [('unetr_conv3_pack_grouped', [{'w': 'cpu+0', 'out': 'pack_cpu+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
             ('unetr_conv3_pack_grouped', [{'w': 'dying+0', 'out': 'pack_dying+0', 'Cin': 2, 'Cout': 2, 'kind': 0}], 1, 0, 77)],
            {}),
           ('refresh skips what torch touched and prunes the dead', [], {'held_before': True, 'pruned': True, 'maintained': False, 'cpu': False}),
           ('refresh: one launch per precision',
            [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
             ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack10+0', 'Cin': 2, 'Cout': 4, 'kind': 1}], 1, 0, 77),
             ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77),
             ('unetr_conv3_pack_grouped',
              [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}, {'w': 'param+1440', 'out': 'pack10+0', 'Cin': 2, 'Cout': 4, 'kind': 1}],
              2,
              0,
              77),
             ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
            {'maintained': [True, True, True], 'cpu': False}),
           ('a new epoch keeps maintained packs', [], {}),
           ('version bump re-packs',
            [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
            {'maintained': [True, True, False]}),
           ('refresh takes only the packs in step',
            [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
            {'maintained': [True, True, True]}),
           ('under capture: maintained never, unmaintained always',
            [('unetr_conv3_pack_grouped', [{'w': 'cpu+0', 'out': 'pack_cpu+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
             ('unetr_conv3_pack_grouped', [{'w': 'cpu+0', 'out': 'pack_cpu+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77)],
            {}),
           ('invalidate: refresh finds nothing in step', [], {}),
           ('invalidate re-packs',
            [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
            {'maintained': False}),
           ('re-pointed .data re-packs', [('unetr_conv3_pack_grouped', [{'w': 'cw2+0', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)], {})],
 'words': [('absent under capture: None, and no arena', [], {'got': None, 'arena': False}),
           ('first use: one launch over the whole arena',
            [('unetr_split_words', 'param+0', 'words+0', 584, 77)],
            {'buf': 'words+0', 'shape': (8, 16), 'dtype': 'torch.int32'}),
           ('every parameter of the arena has its slice', [], {'bias': 'words+1024', 'lone': None}),
           ('version bump re-splits the padded slot; the epoch does not matter', [('unetr_split_words', 'param+1024', 'words+1024', 8, 77)], {}),
           ('a stale slice under capture', [('unetr_split_words', 'param+0', 'words+0', 128, 77)], {}),
           ('refresh, not written: one derive launch, every slice stamped', [('unetr_split_words', 'param+0', 'words+0', 584, 77)], {}),
           ('refresh, written: stamped without a launch', [], {}),
           ('invalidate re-splits', [('unetr_split_words', 'param+512', 'words+512', 128, 77)], {}),
           ('UNETR_AMD_X3_WORDS=0', [], {'got': None}),
           ('a moved parameter has no words', [], {'got': None, 'other': 'words+0'})],
 'twins': [('no armed epilogue: no twin, no arena', [], {'got': None, 'arena': False}),
           ('the bf16 communication epilogue does not count', [], {'got': None, 'arena': False}),
           ('never created under capture', [], {'got': None, 'arena': False}),
           ('armed AdamW epilogue: the arena is created, zero-filled, and the twin derived',
            [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77)],
            {'buf': 'twins+0', 'shape': (16, 8), 'dtype': 'torch.bfloat16', 'zero': True, 'epilogue': True}),
           ('the second weight',
            [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77)],
            {'buf': 'twins+256', 'shape': (8, 16)}),
           ('no twin for 1-D, unaligned, conv or foreign weights', [], {'got': [None, None, None, None]}),
           ('current twins are handed out', [], {}),
           ('prefetch names the twin of a data-gradient GEMM',
            [],
            {'pf': [('twins+0', 256), ('shadow+528', 192)], 'big': [('shadow+0', 256)], 'fwd': [('shadow+0', 256)]}),
           ('an existing arena serves a pass without epilogue', [], {'same': True}),
           ('under capture without epilogue: None', [], {'got': None, 'pf': [('shadow+0', 256)]}),
           ('under capture with it: the current twin', [], {'same': True, 'pf': [('twins+0', 256)]}),
           ('under capture a stale twin is not handed out', [], {'got': None, 'pf': [('shadow+0', 256)]}),
           ('every stale twin of the arena in one grouped launch',
            [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77),
             ('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77),
             ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77)],
            {'unmaintained': 2}),
           ('after invalidate: all of them',
            [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77),
             ('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77),
             ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77)],
            {}),
           ('refresh: a written twin keeps its stamp, the others are re-derived',
            [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77)],
            {}),
           ('written and stale stays stale',
            [('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77),
             ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77)],
            {'pf': [('shadow+256', 256)]}),
           ('the next pass re-derives it', [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77)], {}),
           ('a captured step only marks stale', [], {'pf': [('shadow+0', 256)]}),
           ('and the next eager pass re-derives', [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77)], {}),
           ('refresh with an out-of-step shadow marks stale, derives the rest',
            [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77)],
            {}),
           ('UNETR_AMD_WT=0', [], {'got': None, 'epilogue': None, 'pf': [('shadow+256', 256)]}),
           ('ArenaState.clear drops the arena and its entries', [], {'arena': False, 'pf': [('shadow+256', 256)]}),
           ('a new arena after the drop',
            [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins2+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77)],
            {'buf': 'twins2+256', 'same': False})],
 'trailers': [('warm',
               [('unetr_split_words', 'param+0', 'words+0', 584, 77),
                ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77),
                ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
               {}),
              ('per-tensor step',
               [('unetr_split_words', 'param+0', 'words+0', 584, 77),
                ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('twins+0', 256), ('twins+256', 256)]}),
              ('flat step',
               [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('twins+0', 256), ('twins+256', 256)]}),
              ('fused finish',
               [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('twins+0', 256), ('twins+256', 256)]}),
              ('reduced end',
               [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('twins+0', 256), ('twins+256', 256)]}),
              ('between steps',
               [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77)],
               {'unmaintained': 1, 'packs': [True, True], 'bf16': [False, True], 'twins': [('shadow+0', 256), ('shadow+256', 256)]}),
              ('flat step after torch touched weights',
               [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('twins+0', 256), ('twins+256', 256)]}),
              ('fused finish after torch touched weights',
               [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77),
                ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('shadow+0', 256), ('twins+256', 256)]}),
              ('what the next pass re-derives',
               [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77),
                ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77)],
               {}),
              ('reduced end under capture',
               [('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77)],
               {'unmaintained': 0, 'packs': [True, True], 'bf16': [True, True], 'twins': [('shadow+0', 256), ('shadow+256', 256)]})],
 'listing': [('warm',
              [('unetr_split_words', 'param+0', 'words+0', 584, 77),
               ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}], 1, 77),
               ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 128, 'N': 16, 'K': 8}], 1, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
              {}),
             ('before a step: maintained arena shadows and the words; neither the cast shadow nor the packs',
              [('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77)],
              {'as_is': [('bf16', 'param+0'),
                         ('x3', 'param+0'),
                         ('bf16', 'param+512'),
                         ('x3', 'param+512'),
                         ('bf16', 'param+1024'),
                         ('x3', 'param+1024'),
                         ('bf16', 'param+1056'),
                         ('x3', 'param+1056'),
                         ('bf16', 'param+1440'),
                         ('x3', 'param+1440'),
                         ('bf16', 'param+2304'),
                         ('x3', 'param+2304')],
               'listed': [('bf16', 'param+0'),
                          ('x3', 'param+0'),
                          ('bf16', 'param+512'),
                          ('x3', 'param+512'),
                          ('bf16', 'param+1024'),
                          ('x3', 'param+1024'),
                          ('bf16', 'param+1056'),
                          ('x3', 'param+1056'),
                          ('bf16', 'param+1440'),
                          ('x3', 'param+1440'),
                          ('bf16', 'param+2304'),
                          ('x3', 'param+2304'),
                          ('bf16', 'lone+0'),
                          ('pack', 'param+1440', 0, 0),
                          ('pack', 'param+1440', 0, 1)]}),
             ('after a step: everything',
              [('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
              {'as_is': [('bf16', 'param+0'),
                         ('x3', 'param+0'),
                         ('bf16', 'param+512'),
                         ('x3', 'param+512'),
                         ('bf16', 'param+1024'),
                         ('x3', 'param+1024'),
                         ('bf16', 'param+1056'),
                         ('x3', 'param+1056'),
                         ('bf16', 'param+1440'),
                         ('x3', 'param+1440'),
                         ('bf16', 'param+2304'),
                         ('x3', 'param+2304'),
                         ('bf16', 'lone+0'),
                         ('pack', 'param+1440', 0, 0),
                         ('pack', 'param+1440', 0, 1)]}),
             ('torch touched a weight: its shadow and words drop out',
              [],
              {'as_is': [('bf16', 'param+512'),
                         ('x3', 'param+512'),
                         ('bf16', 'param+1024'),
                         ('x3', 'param+1024'),
                         ('bf16', 'param+1056'),
                         ('x3', 'param+1056'),
                         ('bf16', 'param+1440'),
                         ('x3', 'param+1440'),
                         ('bf16', 'param+2304'),
                         ('x3', 'param+2304'),
                         ('bf16', 'lone+0'),
                         ('pack', 'param+1440', 0, 0),
                         ('pack', 'param+1440', 0, 1)]}),
             ('refresh re-derives what the graph reads as it is; nothing moved',
              [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77), ('unetr_split_words', 'param+0', 'words+0', 128, 77)],
              {'ok': True, 'same': True}),
             ('the next call starts an epoch: the copy that is no longer maintained is re-derived again',
              [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77)],
              {'ok': True}),
             ('after invalidate: every as-is copy',
              [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77),
               ('unetr_split_words', 'param+0', 'words+0', 128, 77),
               ('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77),
               ('unetr_split_words', 'param+512', 'words+512', 128, 77),
               ('unetr_cast_bf16', 'param+1024', 'shadow+512', 5, 77),
               ('unetr_split_words', 'param+1024', 'words+1024', 8, 77),
               ('unetr_cast_bf16', 'param+1056', 'shadow+528', 96, 77),
               ('unetr_split_words', 'param+1056', 'words+1056', 96, 77),
               ('unetr_cast_bf16', 'param+1440', 'shadow+720', 216, 77),
               ('unetr_split_words', 'param+1440', 'words+1440', 216, 77),
               ('unetr_cast_bf16', 'param+2304', 'shadow+1152', 8, 77),
               ('unetr_split_words', 'param+2304', 'words+2304', 8, 77),
               ('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
              {'ok': True,
               'as_is': [('x3', 'param+0'), ('x3', 'param+512'), ('x3', 'param+1024'), ('x3', 'param+1056'), ('x3', 'param+1440'), ('x3', 'param+2304')]}),
             ('a parameter moved: capture again',
              [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77),
               ('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77),
               ('unetr_cast_bf16', 'param+1024', 'shadow+512', 5, 77),
               ('unetr_cast_bf16', 'param+1056', 'shadow+528', 96, 77),
               ('unetr_cast_bf16', 'param+1440', 'shadow+720', 216, 77),
               ('unetr_cast_bf16', 'param+2304', 'shadow+1152', 8, 77),
               ('unetr_cast_bf16', 'lone+0', 'sh_lone+0', 64, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77)],
              {'ok': False}),
             ('the new capture is stable',
              [],
              {'ok': True,
               'as_is': [('x3', 'param+0'), ('x3', 'param+512'), ('x3', 'param+1024'), ('x3', 'param+1056'), ('x3', 'param+1440'), ('x3', 'param+2304')]}),
             ('a derived buffer moved: the signature differs there only', [('unetr_cast_bf16', 'lone+0', 'sh_lone4+0', 32, 77)], {'diff': [6, 20], 'n': 23}),
             ('refresh_derived_weights: bf16, words, packs, then the twins',
              [('unetr_cast_bf16', 'param+0', 'shadow+0', 128, 77),
               ('unetr_split_words', 'param+0', 'words+0', 128, 77),
               ('unetr_cast_bf16', 'param+512', 'shadow+256', 128, 77),
               ('unetr_split_words', 'param+512', 'words+512', 128, 77),
               ('unetr_cast_bf16', 'param+1024', 'shadow+512', 5, 77),
               ('unetr_cast_bf16', 'param+1056', 'shadow+528', 96, 77),
               ('unetr_cast_bf16', 'param+1440', 'shadow+720', 216, 77),
               ('unetr_split_words', 'param+1440', 'words+1440', 216, 77),
               ('unetr_cast_bf16', 'param+2304', 'shadow+1152', 8, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack00+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 0, 77),
               ('unetr_conv3_pack_grouped', [{'w': 'param+1440', 'out': 'pack01+0', 'Cin': 2, 'Cout': 4, 'kind': 0}], 1, 1, 77),
               ('unetr_transpose_bf16_grouped', 'shadow+0', 'twins+0', [{'offset': 0, 'N': 8, 'K': 16}, {'offset': 128, 'N': 16, 'K': 8}], 2, 77)],
              {}),
             ('and nothing when all is current', [], {})]}
